// api_static.hip -- the static least-squares path: the reference's dispatcher resolved into a SolvePlan, a pure route picker over the
// frame's shape, and one function per route (see the table of static routes in DESIGN.md).  Host code only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "common.hpp"
#include "api_internal.hpp"
#include "k1_gram_chol.hpp"
#include "k2_resident.hpp"
#include "k2w_resident.hpp"
#include "k5_enet.hpp"
#include "k6_svd.hpp"
#include "k8_wide.hpp"
#include "../../include/pols_mi355x_debug.h"

namespace pols {
template <typename T> bool k1m_fits(int k_user, bool has_w, int64_t max_rows);   // k1m_f32.hip / k1m_f64.hip

// ------------------------------------------------------------------ the solve plan
// Dispatcher of src/expressions.rs:366-387.  (solve_method "chol" / "lu" with alpha == 0 go through solve_ridge(alpha = 0), ex.rs:366-376: the
// RIDGE branch.)
int resolve_solve_plan(const pols_ols_params *p, int dtype, int kt, int n_targets, SolvePlan *out) {
    const int m = p->solve_method;
    const double alpha = p->alpha;
    const bool positive = p->positive != 0, multi = n_targets > 1;
    SolvePlan s;
    if (alpha == 0.0 && !positive && (m == POLS_SOLVE_AUTO || m == POLS_SOLVE_SVD || m == POLS_SOLVE_QR)) {
        s.branch = SolveBranch::Ols;   // solve_ols: QR / SVD least squares == normal-equation solution for full column rank
    } else if (alpha >= 0.0 && (p->has_l1_ratio ? p->l1_ratio : 0.0) == 0.0 && !positive) {
        if (!(m == POLS_SOLVE_AUTO || m == POLS_SOLVE_CHOL || m == POLS_SOLVE_LU || m == POLS_SOLVE_SVD))
            return fail(POLS_ERR_PANIC, "Only 'Cholesky', 'LU', & 'SVD' are currently supported solver methods for Ridge.");  // ls.rs:366
        s.branch = SolveBranch::Ridge;
        s.ridge_alpha = alpha;
    } else {
        if (!(m == POLS_SOLVE_AUTO || m == POLS_SOLVE_CD || m == POLS_SOLVE_CD_ACTIVE_SET))
            return fail(POLS_ERR_PANIC, "Only solve_method 'CD' (coordinate descent) is currently supported for Elastic Net / Lasso problems.");  // ls.rs:404
        if (!(alpha > 0.0)) return fail(POLS_ERR_PANIC, "'alpha' must be strictly positive");  // ls.rs:409
        const double l1 = p->has_l1_ratio ? p->l1_ratio : 0.5;
        if (!(l1 >= 0.0 && l1 <= 1.0)) return fail(POLS_ERR_PANIC, "'l1_ratio' must be strictly between 0. and 1.");  // ls.rs:410
        s.branch = SolveBranch::Enet;
        s.enet_l1 = l1;
    }
    // OLS branch (the reference solves it with a backward-stable pivoted QR / dgelsd): flag groups whose Cholesky pivots say the
    // normal equations cannot deliver the parity tolerance (1e-6 f64, 1e-4 f32); they go to the fix-up pass.  The thresholds are
    // MEASURED (scripts/cond_ladder.py -> profiles/cond_ladder.txt, DESIGN.md "K6 fix_up"): the smallest half-decade T such that every
    // raw solve of a group with exact pivot ratio >= T / sqrt(10) was within the tolerance on every route -- 10^-1.5 for f32 batches,
    // 1e-6 for f64.  (1e-3 / 1e-10 until then: unflagged groups up to 19 x / 2e4 x outside the tolerance in the one to four decades above them.)
    // Ridge branch: the reference solves the same normal equations in f64, so an f64 batch flags only a failed factorisation; an f32
    // batch also flags pivots that say cond(X'X + alpha I) * eps_f32 would exceed the 1e-4 tolerance -- those groups get the
    // reference's own chain (Cholesky -> LU) in f64 from the fix-up pass, on every route under solve_method None / "chol": the in-kernel
    // LU retry of K2 and of the streamed solve would factor the same f32-born Gram matrix again (measured up to 480 x the tolerance), so
    // f32 batches do not use it.  (An explicit solve_method "lu" on those two routes is still solved in the kernel and flags only what
    // its LU cannot solve: not measured, not covered by the ladder tests.)
    // A pivot within 16 k eps of its diagonal entry is rounding noise around the exact 0 of a singular matrix: it counts as a failed
    // factorisation ("Cholesky decomposition failed, falling back to LU", demo notebook cell 30) rather than a coin flip.
    s.chol_noise = 16.0 * (double)kt * 2.220446049250313e-16;
    const bool f32 = dtype == POLS_F32;
    const double cond_tol = f32 ? 0.03162277660168379 : 1e-6;
    s.pivot_tol = s.ols() ? cond_tol : (f32 && m != POLS_SOLVE_SVD ? cond_tol : s.chol_noise);
    // Singular-value cut-off of the minimum-norm solver, relative to s_max.  OLS branch: dgelsd drops s < eps * s_max (rcond
    // ignored, ls.rs:181-191); the Jacobi rotations leave an exactly dependent column with a norm of a few ulps of s_max rather
    // than 0, so the cut-off sits 8 ulps up -- enough for that noise at the widths where it can be told from signal, far below the
    // ~5e-14-relative direction the reference's test_fit_multi_collinear[99-"svd"] expects to be resolved.  (Exact dependence at
    // tens of columns is a knife edge at this cut-off in LAPACK too; numpy's eps * max(n, k) would settle it and break that
    // test.)  Ridge branch "svd" (and solve_multi_target -> solve_ridge_svd): the caller's rcond, else -1 = eps * max(fit rows,
    // columns) OF THE GROUP, computed in the kernel (solve_ridge_svd, ls.rs:143-145).
    s.rc_factor = s.ols() ? 8.0 * 2.220446049250313e-16 : (((m == POLS_SOLVE_SVD || multi) && p->has_rcond) ? p->rcond : -1.0);
    // ... and the solver itself is the one the reference runs for this (branch, solve_method): solve_ols None -> pivoted QR when
    // n > k else SVD (ls.rs:224-231), "qr" -> QR, "svd" -> SVD; solve_ridge None / "chol" -> Cholesky then LU, "lu" -> LU (:352-363);
    // solve_multi_target (ls.rs:243-260): the SVD forms
    s.fix_mode = s.ols() ? (multi ? FIX_MINNORM : m == POLS_SOLVE_AUTO ? FIX_OLS_AUTO : m == POLS_SOLVE_QR ? FIX_OLS_QR : FIX_MINNORM)
                         : ((m == POLS_SOLVE_SVD || multi) ? FIX_MINNORM : m == POLS_SOLVE_LU ? FIX_LU : FIX_CHOL_LU);
    // solve_ridge (None / "chol"): Cholesky, and on failure LU (ls.rs:358-363), in the kernel for f64 batches; "svd", the OLS branch
    // and f32 batches flag for the fix-up pass
    s.lu_fallback = (s.branch == SolveBranch::Ridge && m != POLS_SOLVE_SVD && !f32) ? 1 : 0;
    *out = s;
    return POLS_OK;
}

int ensure_fallback_epoch(pols_ctx *ctx) {
    if (!ctx->fb_flag) {
        POLS_HIP(hipMalloc(reinterpret_cast<void **>(&ctx->fb_flag), 256));
        POLS_HIP(hipMemsetAsync(ctx->fb_flag, 0, 256, ctx->stream));
    }
    ctx->epoch = (ctx->epoch % 0x0ffffff0) + 1;
    return POLS_OK;
}

// ------------------------------------------------------------------ the route picker
// Shapes the register-resident VALU engine (K1) takes: up to 8 columns whenever the largest group fits its biggest team, and 9-10
// columns (8 features + intercept, the smoke() shape) while every row stays resident in the wave / two-wave kernels whose Gram
// is accumulated in passes -- 10 000 x 1 000 x (8 + 1) f32: 77.8 us = 5.1 TB/s against 110 us for the LDS-tile engine (K1m),
// f64 153.8 against 243.5 us (scripts/bench_k9.py).  nulls: its null-policy family -- up to 8 columns like the plain kernels, 9-15
// columns (masked three- / four-pass Gram) while resident, 16-31 where the plain kernels run.
static bool k1_takes(const Options &opt, bool aligned, bool f32, int kt, int64_t max_rows, bool has_w, bool nulls) {
    const int vec = f32 ? 4 : 2;
    if (kt <= 8 && max_rows <= (int64_t)256 * 2 * vec) return true;
    const int64_t need = max_rows + (aligned ? 0 : vec - 1);
    // round 5: four chunks per lane of the 256-thread team -- up to 4 096 f32 / 2 048 f64 rows stay register-resident at up to 10 columns
    // (9-10 f32 columns used to leave K1 at 1 024 rows for K1m: 3.2 against 5.3 TB/s on 5 000 x 2 000 x (8 + 1)); POLS_K1_RC2_WIDE=0: the old rule
    if (!nulls && kt <= K1_MAX_KT && opt.static_engine != 2) {
        // (f64, 10 columns WITH weights: the four-chunk kernel needs 278 registers -- AGPRs, one wave per SIMD -- and stays with K2)
        if (kt <= 8 || (opt.k1_rc2_wide && !(!f32 && kt == 10 && has_w))) return need <= (int64_t)256 * 4 * vec;
        return need <= 1024;
    }
    if (kt <= K1_MAX_KT) return need <= 1024;
    if (kt <= K1W_MAX_KT) return need <= (int64_t)256 * 2 * vec;   // 11-15 columns: up to the 256-thread team's resident rows
    // 16-31 columns: one chunk per lane.  f64 only where it measured faster than the alternatives (scripts/bench_k16.py, 50 000 x 200
    // rows): 17-24 columns (867 vs 1 189 us at 20, 1 122 vs 1 418 at 24; at 16 K2 wins 433 vs 506, at 31 the 15-pass kernel is down
    // to one wave per SIMD and loses 2 686 vs 1 923)
    if (!nulls && !f32 && kt == 16 && need <= 16 * vec && !opt.k1_notiny) return true;   // (round 5: K1t, four groups per wave: 24-row groups 0.7 TB/s in K2)
    if (!f32 && (kt < 17 || kt > 24)) return false;
    return kt <= K1X_MAX_KT && need <= (int64_t)256 * 1 * vec;
}
bool k1_valu_takes(const Options &opt, bool aligned, bool f32, int kt, int64_t max_rows, bool has_w) {
    return k1_takes(opt, aligned, f32, kt, max_rows, has_w, false);
}

// Everything the route of a static call depends on: plain data, no context, no device.  Of the options the picker reads static_engine,
// k1_engine, no_classes, timeline, k1_persist, k1_rc2_wide, k1_notiny and kg_single_buffer.
struct RouteInputs {
    Options opt;
    int dtype, kt, n_features;
    bool has_w;
    int pol;                                     // the effective null policy ("ignore" when the batch promises there is nothing null)
    SolveBranch branch;
    int solve_method;
    bool has_rcond;
    int64_t n_groups, n_rows, max_rows;
    bool aligned[2];                             // of the offsets scan, like max_rows and ...
    const int64_t *hist_cnt, *hist_rows;         // ... its 48 size buckets (OffsetsScan)
};
static RouteInputs route_inputs(const Options &opt, const pols_batch *b, const pols_ols_params *p, int pol, const SolvePlan &plan, int64_t max_rows,
                                const bool *aligned, const int64_t *hist_cnt, const int64_t *hist_rows) {
    return RouteInputs{opt, b->dtype, b->n_features + (b->add_intercept ? 1 : 0), b->n_features, b->weights != nullptr, pol, plan.branch,
                       p->solve_method, p->has_rcond != 0, b->n_groups, b->n_rows, max_rows, {aligned[0], aligned[1]}, hist_cnt, hist_rows};
}

enum class StaticRoute : int { Wide, SvdAll, K2, K2w, Streamed, ClassesStreamedTop, Classes, K1 };
static const char *route_name(StaticRoute r) {
    static const char *const names[] = {"wide", "svd_all", "k2", "k2w", "streamed", "classes_streamed_top", "classes", "k1"};
    return names[(int)r];
}
struct RoutePick {
    StaticRoute route = StaticRoute::K1;
    int64_t k1_top = 0;          // ClassesStreamedTop: the largest group the K1 family takes; longer ones are streamed
    int64_t cut[3] = {0, 0, 0};  // class c holds the groups of cut[c - 1] < rows <= cut[c], the last one the rest
    int n_cut = 0;
};

// Size-class split of the static K1 path: up to two thresholds t[0] < t[1] (rows), n = how many; 0 = one launch.
// Cost model: a group costs max(rows, 0.5 x the capacity of the kernel its class gets) row-times (fitted to scripts/bench_spread.py -- 0.3 explains the one-launch numbers, 0.5 also cuts the 50 / 50 frame of 30- and 1 000-row groups, 4.6 -> 5.0 TB/s: log-normal sizes
// with a 4 000-row tail 1.5 TB/s, 90 % 50-row + 10 % 1 000-row groups 1.9 TB/s in one launch), an extra launch a fixed 6e5.
static int pick_size_classes(const RouteInputs &in, int64_t max_rows, int64_t *t) {
    const bool f32 = in.dtype == POLS_F32;
    t[0] = t[1] = 0;
    if (in.opt.no_classes || in.n_groups < 2048) return 0;
    const double alpha = 0.5, launch_cost = 6.0e5;                    // (an extra launch: ~5 us of a chip that moves ~1.2e5 rows per us)
    const int b0 = f32 ? 7 : 6;                                       // the smallest kernels hold 128 f32 / 64 f64 rows per group
                                                                      // (cuts at 32 / 16 rows -- K1t's eight-lane teams -- measured no better: the 6-row groups of the mixed frame
                                                                      // are minimum-norm problems anyway, and 50-row groups lost 6 % to the 64-row form)
    int bc = b0;
    while (((int64_t)1 << bc) < max_rows && bc < 46) ++bc;            // capacity of the kernel the largest group asks for: 2^bc rows
    // cost with class boundaries at buckets s0 < s1 (-1: unused): bucket q goes to the first boundary >= q, else to the top kernel
    auto cost = [&](int s0, int s1) {
        double c = launch_cost * ((s0 >= 0) + (s1 >= 0));
        for (int q = 0; q < 48; ++q) {
            if (!in.hist_cnt[q]) continue;
            const double avg = (double)in.hist_rows[q] / (double)in.hist_cnt[q];
            const int kb = (s0 >= 0 && q <= s0) ? s0 : ((s1 >= 0 && q <= s1) ? s1 : bc);
            c += (double)in.hist_cnt[q] * std::max(avg, alpha * (double)((int64_t)1 << kb));
        }
        return c;
    };
    auto count_le = [&](int sb) { int64_t n = 0; for (int q = 0; q <= sb; ++q) n += in.hist_cnt[q]; return n; };
    const double one = cost(-1, -1);
    double best = one;
    int bs0 = -1, bs1 = -1;
    for (int s1 = b0; s1 < bc; ++s1) {
        const int64_t le1 = count_le(s1);
        if (le1 == 0 || le1 == in.n_groups) continue;
        const double c1 = cost(-1, s1);
        if (c1 < best) { best = c1; bs0 = -1; bs1 = s1; }
        for (int s0 = b0; s0 < s1; ++s0) {
            const int64_t le0 = count_le(s0);
            if (le0 == 0 || le0 == le1) continue;
            const double c2 = cost(s0, s1);
            if (c2 < 0.9 * c1 && c2 < best) { best = c2; bs0 = s0; bs1 = s1; }   // (a third launch has to earn its exiting workgroups)
        }
    }
    if (bs1 < 0 || !(best < 0.75 * one)) return 0;
    // (a kernel that holds 2^b rows per group takes ragged groups of up to 2^b - (VEC - 1): the chunk grid starts at the 16-byte boundary below the group)
    const int slack = in.aligned[f32 ? 1 : 0] ? 0 : (f32 ? 3 : 1);
    int n = 0;
    if (bs0 >= 0) t[n++] = ((int64_t)1 << bs0) - slack;
    t[n++] = ((int64_t)1 << bs1) - slack;
    return n;
}

// Which kernel family takes the frame: one ordered rule list, the first rule that holds wins.  Launches nothing, allocates nothing.
// (Every threshold assumes an MI355X: 160 KiB of LDS and 512 VGPRs per SIMD decide what "fits"; nothing here reads the device.)
static RoutePick pick_static_route(const RouteInputs &in) {
    RoutePick r;
    const bool f32 = in.dtype == POLS_F32, enet = in.branch == SolveBranch::Enet, ols = in.branch == SolveBranch::Ols;
    const bool nulls = in.pol != POLS_NULL_IGNORE, aligned = in.aligned[f32 ? 1 : 0];
    const int vec = f32 ? 4 : 2, kt = in.kt, m = in.solve_method;
    const int64_t max_rows = in.max_rows;

    // 32 .. 1024 columns: the K8 kernels
    if (kt > 31) { r.route = StaticRoute::Wide; return r; }

    // solve_ridge_svd with a caller-supplied rcond (ls.rs:143-148): singular values below rcond * s_max are dropped on EVERY
    // group, full rank or not -- a truncated solve is not the normal-equation solution, so the Jacobi-SVD kernel takes all of
    // them (one workgroup per group from a pool of up to 2 048 workers; an opt-in, rarely used form of the call).
    // A whole frame of fewer rows than one 16-byte vector (1-3 f32 / 1 f64 rows) goes the same way: the vector kernels clamp their
    // loads into the columns and need that much to clamp into; the fix-up solvers are the reference's own for every (branch, method).
    const bool tiny_frame = !enet && in.n_rows < vec;
    if (!enet && ((!ols && m == POLS_SOLVE_SVD && in.has_rcond) || tiny_frame)) { r.route = StaticRoute::SvdAll; return r; }

    // resident in the K1 family?  (null policies: the register-resident K1 has a NULLS family)
    auto takes = [&](int64_t rows) { return k1_takes(in.opt, aligned, f32, kt, rows, in.has_w, nulls); };
    const bool k1_resident = takes(max_rows);
    const bool fits_lds = f32 ? k1m_fits<float>(in.n_features, in.has_w, max_rows) : k1m_fits<double>(in.n_features, in.has_w, max_rows);

    // K2 (k2_resident.hip): rows resident in registers, X'X on the matrix cores, the solver in the same workgroup -- X is read
    // once whatever the solver.  Elastic net / lasso, explicit LU, and OLS / ridge beyond K1's eight columns or resident rows,
    // whenever the largest group fits; POLS_STATIC_ENGINE=stream | nok2 go back to the three-launch path / K1m.
    {
        const bool k2_ok = !nulls && kt <= K2_KMAX && k2_fits(in.dtype, kt, max_rows, aligned) && in.n_rows >= vec && in.opt.static_engine != 1 &&
                           in.opt.static_engine != 3;
        // (the eight-wave forms are ONE persistent workgroup per CU sized for the largest group: a frame whose groups mostly fill a fraction of it --
        // log-normal sizes around 300 rows with a 4 000-row tail: 1.07 TB/s in the four-chunk form -- is better off on the streamed path, 2.9;
        // elastic net keeps K2: its solve needs the rows once)
        const int64_t k2_cap = max_rows > (int64_t)512 * 2 * vec ? (int64_t)512 * 4 * vec : (int64_t)512 * 2 * vec;
        const bool k2_sparse = !enet && in.opt.static_engine != 2 && max_rows > (int64_t)256 * 2 * vec && in.n_groups >= 2048 &&
                               (double)in.n_rows < 0.3 * (double)k2_cap * (double)in.n_groups;
        // POLS_K1_ENGINE=valu | mfma keep the K1 / K1m kernels reachable for the shapes they cover (A/B measurements, tests)
        const bool legacy_forced = (in.opt.k1_engine == 2 && kt <= K1M_MAX_KT) || (in.opt.k1_engine == 1 && kt <= K1_MAX_KT);
        // OLS / ridge with 9..15 columns whose tile fits LDS stay with K1m: its solve runs unrolled on wave-uniform values in every
        // lane (~1.5k cycles), K2's lane-cooperative register Cholesky pays ~40 cycles per cross-lane broadcast (11k cycles at 16
        // padded columns) -- measured 3.7 against 1.6 TB/s on 10 000 x 1 000 x (8 + intercept) f32.  K2 takes what K1m cannot:
        // 16 columns, tiles beyond LDS, and every solver that is not a Cholesky.
        const bool k1m_takes = kt <= K1M_MAX_KT && fits_lds;
        // Round 3: K2's loop lost its per-column wave-uniform branches and skips the tile stages of chunks a wave has no row of; on the
        // over-resident shapes (rows beyond K1's registers, tile within LDS) it now beats K1m everywhere measured but f32 with 9-10
        // columns -- f64 9 / 12 / 15 columns x 1 100 rows: 434 / 447 / 455 us against 468 / 562 / 722; f32 x 2 200 rows: 358 / 364 / 366
        // against 306 / 371 / 442 (profiles/r03_ab_overresident.txt).
        // Round 5, re-measured at 8 columns (f32 groups of 2 049..4 096 rows -- ten years of trading days per asset): K2 wins there too, 0.165 /
        // 0.143 / 0.119 ms against K1m's 0.189 / 0.177 / 0.156 on 4 000 x 2 500, 3 333 x 3 000 and 2 500 x 4 000 rows; K1m keeps 9-10 columns.
        const bool k1m_wins = k1m_takes && f32 && kt >= 9 && kt <= 10;
        const bool want = enet || m == POLS_SOLVE_LU || in.opt.static_engine == 2 || (!k1_resident && !legacy_forced && !k1m_wins);
        if (k2_ok && want && !k2_sparse) { r.route = StaticRoute::K2; return r; }
    }

    // K2w (k2w_kernel.inl): OLS / ridge with 17..31 columns, rows resident in registers, Z'Z as three 16 x 16 tiles on the matrix cores,
    // Cholesky in the same workgroup -- X read ONCE for groups of up to 1 024 f64 / 2 048 f32 rows, which the three-launch streamed
    // path below reads twice.  Takes what the resident K1 kernels do not (their shapes: k1_valu_takes); POLS_STATIC_ENGINE=k2w takes
    // every shape it fits (A/B), =stream / =nok2 leave it out.
    {
        const bool fits = !enet && !nulls && m != POLS_SOLVE_LU && k2w_fits(in.dtype, kt, max_rows, aligned) && in.n_rows >= vec &&
                          in.opt.static_engine != 1 && in.opt.static_engine != 3;
        // where it measured ahead of the streamed path (scripts/bench_k16.py, 1 000-row groups): f64 from 25 columns (31: 2.45 vs 2.07
        // TB/s; 20: 1.93 vs 2.10 -- one group per CU, and the serial 32-column solve is 40 % of a group's time whatever kt), f32 always
        // (2.53 vs 1.75 at 31 columns)
        // (round 3, solvers padded to 20 / 24 / 28 / 32 and built by independent loads: f64 17 / 20 / 24 columns x 1 000 rows 689 / 722 /
        // 409 us against 729 / 837 / 492 streamed -- ahead at every width it covers now)
        // (round 4, two-wave workgroups -- four per CU, four solves in flight: f64 groups of up to 256 rows 24 / 31 columns x 200 rows
        // 2.03 / 2.10 TB/s against 1.83 (K1) / 1.25 (four waves); at 20 columns K1 stays ahead, 2.02 against 1.87)
        // (round 5, re-measured over 128 .. 512 rows, scripts/ab_wide_f64.py -> profiles/r05_ab_wide_f64.txt: at 23-24 columns K2w is ahead at every length
        // K1 would take (256 rows 0.310 vs 0.404 ms, 512 rows 0.263 vs 0.378), at 22 from ~200 rows (0.396 vs 0.419; 512: 0.256 vs 0.333), at 20-21 from
        // 256 (0.268 vs 0.293; 512: 0.253 vs 0.297); at 17-19 and for groups of ~128 rows K1 stays ahead)
        // (round 6: groups of 257 .. 512 rows take K1's 256-thread team, which runs three waves per SIMD from 18 columns now -- shorter Gram passes, the
        // solving wave's rows parked in LDS: 500 rows x 20 / 21 / 22 columns 2.87 / 2.90 / 3.01 TB/s against 2.4-2.8 for K2w; 23 columns 2.88 vs 2.85 at 500 rows, 1.95 vs 1.76 at 300,
        // profiles/r06_bench_wide_f64_short.txt)
        const bool short_wide = !f32 && (max_rows > 256 ? kt >= 24 : (kt >= 23 || (kt == 22 && max_rows >= 192) || (kt >= 20 && max_rows >= 224)));
        if (fits && (!k1_resident || short_wide || in.opt.static_engine == 4)) { r.route = StaticRoute::K2w; return r; }
    }

    // Streamed three-launch path: elastic net / 16..31 features when the group does not fit K2's registers; OLS / ridge when
    // it fits neither the fused kernels nor K1m's LDS tile.  POLS_STATIC_ENGINE=stream forces it.
    bool stream = enet;
    if (!enet) {
        // null policies: the register-resident K1 has a NULLS family; everything else goes through the streamed kernels
        stream = (nulls && !k1_resident) || (!k1_resident && (kt > K1M_MAX_KT || !fits_lds));
        // Round 5: with the VALU Gram pass (K5v) and the lean prediction kernel the two-pass path runs at 2.7-3.1 TB/s of algorithmic bytes
        // on frames of up to ten columns without a null policy, K1m's LDS-resident single pass at 1.5-2.2 (profiles/r05_sweep_stream_ab.txt): K1m and K1's
        // streamed-overflow form stay reachable through POLS_K1_ENGINE=mfma | valu
        const bool k5v_ok = !nulls && kt <= K5V_MAX_KT && !in.opt.kg_single_buffer && in.opt.k1_engine == 0;
        stream = stream || (!k1_resident && k5v_ok);
        stream = stream || in.opt.static_engine == 1;
        stream = stream || (m == POLS_SOLVE_LU && kt > K1M_MAX_KT);   // explicit LU beyond K2's 16 columns: the streamed solver has one
    }

    // ---- SIZE CLASSES.  The K1 family sizes its workgroup for the LARGEST group of the frame, so on a panel whose group sizes spread widely
    // (most assets a few hundred rows, a few of them thousands) every small group paid for a team it did not fill -- log-normal sizes around
    // 300 rows with a 4 000-row tail 1.5 TB/s, 90 % 50-row + 10 % 1 000-row groups 1.9 (scripts/bench_spread.py).  Such frames get one launch per
    // size class: each walks the list of its own groups with the kernel the dispatcher picks for the class' largest group.  The cuts come
    // from the size histogram of the offsets scan and a two-parameter cost model (pick_size_classes).  When the largest groups do not fit the
    // K1 family at all, they form a class of their own on the streamed path and the rest is classed as above.
    const bool classes_allowed = !enet && !in.opt.no_classes && !in.opt.timeline && in.opt.k1_persist <= 0 && in.opt.static_engine == 0 &&
                                 in.opt.k1_engine == 0 && in.n_groups >= 2048 && in.n_groups <= 0x7fffffffLL && m != POLS_SOLVE_LU;
    if (stream) {
        // the largest groups leave the K1 family: do the others fit it, and are they worth their own launches?
        int64_t k1_top = 0;
        if (classes_allowed && !k1_resident) {
            const int slack = aligned ? 0 : (f32 ? 3 : 1);
            for (int bb = 13; bb >= (f32 ? 7 : 6) && k1_top == 0; --bb)
                if (((int64_t)1 << bb) - slack < max_rows && takes(((int64_t)1 << bb) - slack)) k1_top = ((int64_t)1 << bb) - slack;
            int64_t rows_low = 0;
            for (int q = 0; q < 48 && k1_top > 0; ++q)
                if (((int64_t)1 << q) <= k1_top + 3) rows_low += in.hist_rows[q];
            if ((double)rows_low < 0.3 * (double)in.n_rows) k1_top = 0;      // (mostly long groups: the streamed path for all of them, as before)
        }
        if (k1_top == 0) { r.route = StaticRoute::Streamed; return r; }
        r.route = StaticRoute::ClassesStreamedTop;
        r.k1_top = k1_top;
        r.n_cut = pick_size_classes(in, k1_top, r.cut);
        r.cut[r.n_cut++] = k1_top;
        return r;
    }
    r.n_cut = (classes_allowed && k1_resident) ? pick_size_classes(in, max_rows, r.cut) : 0;
    r.route = r.n_cut > 0 ? StaticRoute::Classes : StaticRoute::K1;
    return r;
}

// ------------------------------------------------------------------ one call, one function per route
// What the routes of one call share: the call itself, its staged columns, the resolved policy, and the fix-up pass' arguments once prepared.
struct StaticCall {
    pols_ctx *ctx;
    const pols_batch *b;
    const pols_ols_params *p;
    pols_out *o;
    Staged st;
    const int64_t *d_offs = nullptr;
    int64_t max_rows = 0;
    int kt = 0, pol = POLS_NULL_IGNORE;          // pol: the effective null policy
    SolvePlan plan;
    K6Args ka;                                   // prepare_fix
    int fix_workers = 0;
    double *stream_gram = nullptr;               // run_stream over the whole frame: the Gram matrices it produced
};

// The block every argument struct of the static path starts from: target, weights, feature columns (slots up to x_slots padded with
// the target: any loadable column), k_user ...
template <typename A>
static void fill_columns(A &a, const StaticCall &c, int x_slots = 0) {
    std::memset(&a, 0, sizeof(a));
    a.y = c.st.y; a.w = c.st.w;
    for (int j = 0; j < std::max(c.b->n_features, x_slots); ++j) a.x[j] = j < c.b->n_features ? c.st.x[j] : c.st.y;
    a.k_user = c.b->n_features;
}
// ... and, for the kernels that solve: the frame's groups, the outputs, the fall-back word and this call's epoch
template <typename A>
static void fill_solve_args(A &a, const StaticCall &c, int x_slots = 0) {
    fill_columns(a, c, x_slots);
    a.offs = c.d_offs; a.n_groups = c.b->n_groups;
    a.coef = c.st.coef; a.pred = c.st.pred; a.resid = c.st.resid; a.status = c.st.status;
    a.fb_flag = c.ctx->fb_flag; a.epoch = c.ctx->epoch;
}

// Arguments + work area of the fix-up pass.
// (the pool of fix-up workgroups: 64 for the frames the benchmarks visit -- an empty dispatch -- growing with the number of groups up to
//  2 048: a frame of a million 10-row f32 groups has most of them re-solved in f64 here, 64 workgroups were a quarter of the chip)
static int prepare_fix(StaticCall &c, int max_workers = 0) {
    const pols_batch *b = c.b;
    if (max_workers <= 0) max_workers = (int)std::max<int64_t>(64, std::min<int64_t>(2048, b->n_groups / 128));
    const int workers = (int)std::min<int64_t>(b->n_groups, max_workers);
    const int64_t stride = std::max<int64_t>(1, c.max_rows) * (c.kt + 1);
    void *wk = nullptr;
    int w_use = workers;
    while (w_use > 1 && (double)w_use * (double)stride * 8.0 > 4e9) w_use /= 2;
    int rc;   // Work::Gram holds the Gram matrices / coef64 of the streamed path: the work area gets its own buffer
    if ((rc = ensure_scratch(c.ctx, Work::Fixup, sizeof(double) * (size_t)w_use * (size_t)stride, &wk))) return rc;
    fill_solve_args(c.ka, c);
    c.ka.work = static_cast<double *>(wk); c.ka.work_stride = stride;
    c.ka.alpha = c.plan.ridge_alpha;
    c.ka.rc_factor = c.plan.rc_factor;
    c.ka.mode = c.plan.fix_mode;
    c.ka.kt = c.kt;
    c.ka.valid = c.st.valid; c.ka.null_policy = c.pol;
    c.fix_workers = w_use;
    return POLS_OK;
}
static int svd_fixup(StaticCall &c) {
    if (c.plan.enet()) return POLS_OK;
    // (measurement aid, an Options switch like the others -- no compute entry reads the environment: what the fix-up dispatch of a
    // call that flags nothing costs on the stream)
    if (c.ctx->opt.debug_skip_fixup) return POLS_OK;
    int rc = prepare_fix(c);
    if (rc) return rc;
    return k6_launch(c.ctx, c.b->dtype, c.ka, c.fix_workers);
}

static int route_svd_all(StaticCall &c) {
    int rc;
    if ((rc = prepare_fix(c, 2048))) return rc;
    hipLaunchKernelGGL(mark_fallback_kernel, dim3((unsigned)((c.b->n_groups + 255) / 256)), dim3(256), 0, c.ctx->stream, c.d_offs,
                       c.b->n_groups, c.st.status, c.ctx->fb_flag, c.ctx->epoch, 0);
    POLS_HIP(hipGetLastError());
    c.ctx->last_kernel = "k6_small_svd_all_groups";
    return k6_launch(c.ctx, c.b->dtype, c.ka, c.fix_workers);
}

static int route_k2(StaticCall &c) {
    const pols_ols_params *p = c.p;
    const bool enet = c.plan.enet();
    K2Args a;
    fill_solve_args(a, c, K2_KMAX);
    a.n_rows = c.b->n_rows; a.kt = c.kt;
    a.solver = enet ? (p->solve_method == POLS_SOLVE_CD_ACTIVE_SET ? K2_CD_ACTIVE_SET : K2_CD) : (p->solve_method == POLS_SOLVE_LU ? K2_LU : K2_CHOL);
    a.lu_fallback = c.plan.lu_fallback;
    a.alpha = enet ? p->alpha : c.plan.ridge_alpha;
    a.l1_ratio = c.plan.enet_l1; a.tol = p->tol; a.max_iter = p->max_iter; a.positive = p->positive ? 1 : 0;
    a.pivot_tol = c.plan.in_kernel_pivot_tol();
    if (enet) a.fb_flag = nullptr;
    int rc = k2_launch(c.ctx, c.b->dtype, a, c.max_rows);
    return rc ? rc : svd_fixup(c);
}

static int route_k2w(StaticCall &c) {
    K2wArgs a;
    fill_solve_args(a, c, 32);
    a.n_rows = c.b->n_rows; a.kt = c.kt;
    a.alpha = c.plan.ridge_alpha; a.pivot_tol = c.plan.pivot_tol;
    int rc = k2w_launch(c.ctx, c.b->dtype, a, c.max_rows);
    return rc ? rc : svd_fixup(c);
}

// The streamed path over the whole frame (ids == nullptr), or over a LIST of its groups (size classes: the groups beyond the K1 family's
// registers; segment tables with (start, end) pairs, Gram matrices / coef64 indexed by list position, gram_solve maps back to group ids).
// One streaming Gram pass, the small solve (Gram-form CD or Cholesky), then (only if asked for) a prediction pass.
static int run_stream(StaticCall &c, const std::vector<int32_t> *ids, const int32_t *d_ids, int64_t class_key, int64_t cls_max_rows) {
    pols_ctx *ctx = c.ctx;
    const pols_batch *b = c.b;
    const pols_ols_params *p = c.p;
    const Staged &st = c.st;
    const bool nulls = c.pol != POLS_NULL_IGNORE;
    const int kt = c.kt;
    int rc;
    const int64_t ng = ids ? (int64_t)ids->size() : b->n_groups;
    const int64_t mr = ids ? cls_max_rows : c.max_rows;
    const size_t nz = (size_t)kt + 1;
    // Few long groups (ONE regression over a whole frame is the reference's first README example): a group is one workgroup in
    // the Gram and the prediction pass, so a 10M-row group used to be one CU's work -- 94 ms.  Long groups are cut into segments
    // (segment offsets, one workgroup each; the segments' Gram matrices are summed per group in segment order), sized so that the
    // launch fills the chip about eight deep.
    SegTables sg;
    if ((rc = ensure_segments(ctx, b, mr, sizeof(double) * (nz * nz + 1), &sg, ids, class_key))) return rc;
    const bool split = sg.n_seg > 0;
    // few groups of hundreds of segments: the segment sums go through 16 slices per group (gram_reduce_launch)
    const int n_slices = (split && sg.max_seg >= 256 && ng <= 256) ? 16 : 1;
    double *gram = nullptr, *coef64 = nullptr, *nvalid = nullptr, *slices = nullptr;
    Carve cv;
    cv.keep(gram, sizeof(double) * nz * nz * (size_t)ng);
    cv.keep(coef64, sizeof(double) * (size_t)kt * (size_t)ng);
    cv.add(nvalid, nulls ? sizeof(double) * (size_t)b->n_groups : 0);
    cv.add(slices, n_slices > 1 ? sizeof(double) * nz * nz * (size_t)n_slices * (size_t)ng : 0);
    if ((rc = carve(ctx, Work::Gram, cv))) return rc;
    const int64_t *seg_offs = split ? sg.offs : c.d_offs;
    const int64_t n_seg = split ? sg.n_seg : ng;
    double *gram_part = reinterpret_cast<double *>(sg.extra);
    double *nv_part = (split && nulls) ? gram_part + nz * nz * (size_t)n_seg : nullptr;
    GramArgs ga;
    fill_columns(ga, c);
    ga.offs = seg_offs; ga.n_groups = n_seg; ga.n_rows = b->n_rows; ga.offs_pairs = ids ? 1 : 0;
    ga.gram = split ? gram_part : gram;
    ga.kt = kt;
    ga.valid = st.valid; ga.null_policy = c.pol; ga.nvalid = split ? nv_part : nvalid;
    if ((rc = gram_stream_launch(ctx, b->dtype, ga))) return rc;
    if (split) {
        GramReduceArgs ra;
        std::memset(&ra, 0, sizeof(ra));
        ra.part = gram_part; ra.nv_part = nv_part; ra.first = sg.first;
        ra.gram = gram; ra.nvalid = nvalid; ra.n_groups = ng; ra.nz2 = (int32_t)(nz * nz);
        ra.max_segments = (int32_t)std::min<int64_t>(1 << 30, sg.max_seg);
        if (n_slices > 1) { ra.slices = slices; ra.n_slices = n_slices; }
        if ((rc = gram_reduce_launch(ctx, ra))) return rc;
        ga.gram = gram;
        ctx->last_kernel += "_split";
    }
    CdArgs ca;
    std::memset(&ca, 0, sizeof(ca));
    ca.gram = ga.gram; ca.offs = c.d_offs; ca.n_groups = ng; ca.glist = d_ids;
    ca.coef = st.coef; ca.coef64 = coef64;
    ca.status = st.status;
    ca.alpha = p->alpha; ca.l1_ratio = c.plan.enet_l1; ca.tol = p->tol; ca.max_iter = p->max_iter;
    ca.positive = p->positive ? 1 : 0; ca.active_set = (p->solve_method == POLS_SOLVE_CD_ACTIVE_SET) ? 1 : 0; ca.kt = kt;
    ca.nvalid = nvalid;
    if (c.plan.enet()) {
        if ((rc = gram_cd_launch(ctx, b->dtype, ca))) return rc;
    } else {
        ca.alpha = c.plan.ridge_alpha;
        ca.solver = (p->solve_method == POLS_SOLVE_LU) ? 1 : 0;
        ca.lu_fallback = c.plan.lu_fallback;
        ca.pivot_tol = c.plan.in_kernel_pivot_tol();
        ca.fb_flag = ctx->fb_flag; ca.epoch = ctx->epoch;
        if ((rc = gram_solve_launch(ctx, b->dtype, ca))) return rc;
    }
    if (st.pred || st.resid) {
        PredictArgs pa;
        fill_columns(pa, c);
        pa.offs = seg_offs; pa.n_groups = n_seg; pa.n_rows = b->n_rows; pa.gmap = sg.map; pa.offs_pairs = ids ? 1 : 0;
        pa.max_item_rows = split ? sg.max_len : mr;
        pa.coef64 = ca.coef64; pa.pred = st.pred; pa.resid = st.resid;
        pa.kt = kt;
        pa.valid = st.valid; pa.null_policy = c.pol;
        if ((rc = predict_launch(ctx, b->dtype, pa))) return rc;
    }
    c.stream_gram = ga.gram;
    return POLS_OK;
}

static int route_streamed(StaticCall &c) {
    int rc = run_stream(c, nullptr, nullptr, 0, 0);
    return rc ? rc : svd_fixup(c);
}

// the lists of the classes cut[0] < cut[1] < ... (rows), cached per frame in ctx->class_cache
static int build_lists(StaticCall &c, const int64_t *cut, int n_cut) {
    pols_ctx *ctx = c.ctx;
    const pols_batch *b = c.b;
    auto &cc = ctx->class_cache;
    bool same = cc.valid && cc.offs_id == ctx->offs_id && cc.n_cut == n_cut;
    for (int i = 0; i < n_cut && same; ++i) same = cc.cut[i] == cut[i];
    if (same) return POLS_OK;
    cc.valid = false;
    std::vector<int32_t> lists[4];
    for (int64_t g = 0; g < b->n_groups; ++g) {
        const int64_t n = b->group_offsets[g + 1] - b->group_offsets[g];
        int i = 0;
        while (i < n_cut && n > cut[i]) ++i;
        lists[i].push_back((int32_t)g);
    }
    void *d = nullptr;
    int rc = grow(cc, sizeof(int32_t) * (size_t)b->n_groups, &d);
    if (rc) return rc;
    size_t at = 0;
    for (int i = 0; i <= n_cut; ++i) {
        if (!lists[i].empty() && (rc = upload_small(ctx, static_cast<int32_t *>(d) + at, lists[i].data(), sizeof(int32_t) * lists[i].size()))) return rc;
        cc.n[i] = (int64_t)lists[i].size();
        at += lists[i].size();
    }
    for (int i = n_cut + 1; i < 4; ++i) cc.n[i] = 0;
    cc.host_last.swap(lists[n_cut]);
    cc.valid = true; cc.offs_id = ctx->offs_id; cc.n_cut = n_cut;
    for (int i = 0; i < n_cut; ++i) cc.cut[i] = cut[i];
    return POLS_OK;
}

static void k1_args(K1Args &a, const StaticCall &c) {
    fill_solve_args(a, c);
    a.valid = c.st.valid;
    a.n_rows = c.b->n_rows;
    a.alpha = c.plan.ridge_alpha;
    a.pivot_tol = c.plan.pivot_tol;
    a.null_policy = c.pol;
}

// K1 launches for the classes [c_lo, c_hi] of the cached lists, longest groups first (their workgroups take longest)
// (Tried: every launch over ALL groups, the workgroups of the other classes exiting after reading their offsets -- 18 000 exits per launch on
// the log-normal frame cost more than the lists' indirection; and the long groups' launch on a second stream beside the short groups' --
// slower by the two events, 0.136 against 0.124 ms.)
static int launch_k1_classes(StaticCall &c, const int64_t *cut, int n_cut, int c_lo, int c_hi, std::string &names) {
    const auto &cc = c.ctx->class_cache;
    K1Args a;
    k1_args(a, c);
    int64_t first[4] = {0, cc.n[0], cc.n[0] + cc.n[1], cc.n[0] + cc.n[1] + cc.n[2]};
    for (int i = c_hi; i >= c_lo; --i) {
        if (cc.n[i] == 0) continue;
        K1Args ac = a;
        ac.glist = static_cast<const int32_t *>(cc.buf.ptr) + first[i];
        ac.n_groups = cc.n[i];
        ac.class_max_rows = i < n_cut ? cut[i] : c.max_rows;
        int rc = k1_launch(c.ctx, c.b->dtype, c.kt, ac, ac.class_max_rows, true);
        if (rc) return rc;
        names += (names.empty() ? "" : " | ") + c.ctx->last_kernel;
    }
    return POLS_OK;
}

// the groups beyond k1_top on the streamed path (a class of their own), the rest in K1 launches per size class
static int route_classes_streamed_top(StaticCall &c, const RoutePick &r) {
    pols_ctx *ctx = c.ctx;
    int rc;
    if ((rc = build_lists(c, r.cut, r.n_cut))) return rc;
    if ((rc = prepare_fix(c))) return rc;
    std::string names;
    const auto &cc = ctx->class_cache;
    if (cc.n[r.n_cut] > 0) {
        const int32_t *d_top = static_cast<const int32_t *>(cc.buf.ptr) + (c.b->n_groups - cc.n[r.n_cut]);
        if ((rc = run_stream(c, &cc.host_last, d_top, r.k1_top, c.max_rows))) return rc;
        names = ctx->last_kernel;
    }
    if ((rc = launch_k1_classes(c, r.cut, r.n_cut, 0, r.n_cut - 1, names))) return rc;
    ctx->last_kernel = names;
    c.stream_gram = nullptr;                     // (of the top class only: not the frame's)
    if (ctx->opt.debug_skip_fixup) return POLS_OK;   // (measurement switch, like svd_fixup)
    return k6_launch(ctx, c.b->dtype, c.ka, c.fix_workers);
}

static int route_k1(StaticCall &c, const RoutePick &r) {
    pols_ctx *ctx = c.ctx;
    int rc;
    if ((rc = prepare_fix(c))) return rc;
    if (r.n_cut > 0) {
        if ((rc = build_lists(c, r.cut, r.n_cut))) return rc;
        std::string names;
        if ((rc = launch_k1_classes(c, r.cut, r.n_cut, 0, r.n_cut, names))) return rc;
        ctx->last_kernel = names;
    } else {
        K1Args a;
        k1_args(a, c);
        if ((rc = k1_launch(ctx, c.b->dtype, c.kt, a, c.max_rows, true))) return rc;
    }
    if (ctx->opt.debug_skip_fixup) return POLS_OK;   // (measurement switch, like svd_fixup)
    return k6_launch(ctx, c.b->dtype, c.ka, c.fix_workers);
}

// Null policies (src/expressions.rs:201-296): a null is a NaN; `valid` (optional) additionally drops rows under the
// drop family.  They are fused into the kernels' staging / prediction passes -- no compaction, no copies.
static int effective_null_policy(const pols_batch *b, const pols_ols_params *p, int *pol) {
    if (p->null_policy < POLS_NULL_IGNORE || p->null_policy > POLS_NULL_DROP_WINDOW) return fail(POLS_ERR_INVALID, "unknown null_policy %d", p->null_policy);
    *pol = (b->null_free && !b->valid) ? POLS_NULL_IGNORE : p->null_policy;   // nothing null: every policy is the identity
    if (b->valid && (*pol == POLS_NULL_IGNORE || *pol == POLS_NULL_ZERO))
        return fail(POLS_ERR_INVALID, "a validity mask needs a drop-family null_policy");
    return POLS_OK;
}

int ls_core(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, pols_out *o, LsInfo *info) {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if ((rc = check_batch(b, o, K8_KMAX))) return rc;
    if (!p) return fail(POLS_ERR_INVALID, "params is NULL");
    StaticCall c{ctx, b, p, o};
    if ((rc = effective_null_policy(b, p, &c.pol))) return rc;
    c.kt = b->n_features + (b->add_intercept ? 1 : 0);
    if ((rc = resolve_solve_plan(p, b->dtype, c.kt, 1, &c.plan))) return rc;
    if (b->n_groups == 0) return POLS_OK;
    if (c.kt > 31) {
        if (info) return fail(POLS_ERR_INVALID, "internal: the wide statistics path calls wide_static itself");
        return wide_static(ctx, b, p, o, c.kt, c.plan);
    }
    if ((rc = upload_offsets(ctx, b->group_offsets, b->n_groups, &c.d_offs, &c.max_rows, b->offsets_generation))) return rc;
    if ((rc = stage_inputs(ctx, b, b->n_groups, c.kt, o, &c.st))) return rc;
    if ((rc = fill_null_weights(ctx, b, &c.st))) return rc;
    // Every static solve is followed by the fix-up pass over the groups it flags, so a status buffer always exists.
    if (!c.plan.enet()) {
        if (!c.st.status) {
            void *sp = nullptr;
            if ((rc = ensure_scratch(ctx, Work::Status, sizeof(int32_t) * (size_t)b->n_groups, &sp))) return rc;
            c.st.status = static_cast<int32_t *>(sp);
        }
        if ((rc = ensure_fallback_epoch(ctx))) return rc;
    }
    const RoutePick r = pick_static_route(route_inputs(ctx->opt, b, p, c.pol, c.plan, c.max_rows, ctx->offs_aligned, ctx->offs_hist_cnt, ctx->offs_hist_rows));
    switch (r.route) {
        case StaticRoute::Wide: return fail(POLS_ERR_INVALID, "internal: wide frames leave before the route picker");
        case StaticRoute::SvdAll: rc = route_svd_all(c); break;
        case StaticRoute::K2: rc = route_k2(c); break;
        case StaticRoute::K2w: rc = route_k2w(c); break;
        case StaticRoute::Streamed: rc = route_streamed(c); break;
        case StaticRoute::ClassesStreamedTop: rc = route_classes_streamed_top(c, r); break;
        case StaticRoute::Classes:
        case StaticRoute::K1: rc = route_k1(c, r); break;
    }
    if (rc) return rc;
    if (!info) return unstage_outputs(ctx, b, b->n_groups, c.kt, o, c.st);
    info->st = c.st; info->d_offs = c.d_offs; info->gram = c.stream_gram;
    return POLS_OK;
}

// ------------------------------------------------------------------ 32 .. 1024 columns
// k8_wide.hip: Gram in 64 x 64 MFMA tiles with row splits, workgroup Cholesky / coordinate descent on the Gram matrix in HBM,
// the fix-up solver for flagged groups, prediction pass.
// Multi-target calls (m > 1) pass the target / prediction column tables; the targets share the Gram matrix and one factorisation.
int wide_static(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, pols_out *o, int kt, const SolvePlan &plan,
                const void *const *y_cols, int m, void *const *pred_cols, WideInfo *info) {
    int rc;
    const bool enet = plan.enet();
    const int64_t *d_offs = nullptr;
    int64_t max_rows = 0;
    if ((rc = upload_offsets(ctx, b->group_offsets, b->n_groups, &d_offs, &max_rows, b->offsets_generation))) return rc;
    Staged st;
    if ((rc = stage_inputs(ctx, b, b->n_groups * m, kt, o, &st))) return rc;
    if ((rc = fill_null_weights(ctx, b, &st))) return rc;
    const size_t G = (size_t)b->n_groups;
    const int NZ = kt + m, nt = (NZ + 63) / 64, npairs = nt * (nt + 1) / 2;
    // multi-target: device pointers of the m target and m prediction columns (host batches are staged in Work::HostStaged)
    std::vector<const void *> yptr;
    std::vector<void *> pptr;
    const bool host = b->mem == POLS_MEM_HOST;
    const size_t colb_mt = round256(dtype_size(b->dtype) * (size_t)b->n_rows);
    if (m > 1) {
        yptr.assign(y_cols, y_cols + m);
        if (pred_cols) pptr.assign(pred_cols, pred_cols + m);
        if (host) {
            char *ys = nullptr, *ps = nullptr;
            Carve mt;
            mt.keep(ys, colb_mt * (size_t)m);
            if (pred_cols) mt.keep(ps, colb_mt * (size_t)m);
            if ((rc = carve(ctx, Work::HostStaged, mt))) return rc;
            for (int t = 0; t < m; ++t) {
                char *yt = column(ys, colb_mt, (size_t)t);
                POLS_HIP(hipMemcpyAsync(yt, y_cols[t], dtype_size(b->dtype) * (size_t)b->n_rows, hipMemcpyHostToDevice, ctx->stream));
                yptr[t] = yt;
                if (pred_cols) pptr[t] = column(ps, colb_mt, (size_t)t);
            }
        }
    }
    const size_t mat = sizeof(double) * (size_t)NZ * NZ;
    // row splits: enough workgroups to fill the chip when there are few groups, bounded by the partial-Gram memory
    int64_t splits = std::max<int64_t>(1, (2048 + (int64_t)G * npairs - 1) / ((int64_t)G * npairs));
    splits = std::min<int64_t>(splits, std::max<int64_t>(1, (max_rows + 255) / 256));
    while (splits > 1 && (double)splits * (double)G * (double)mat > 2e9) splits /= 2;
    int64_t rps = (std::max<int64_t>(1, max_rows) + splits - 1) / splits;
    rps = (rps + 63) / 64 * 64;
    splits = (std::max<int64_t>(1, max_rows) + rps - 1) / rps;

    void *tab = nullptr;
    std::vector<const void *> table(st.x.begin(), st.x.end());         // [features][targets][predictions]
    table.insert(table.end(), yptr.begin(), yptr.end());
    table.insert(table.end(), pptr.begin(), pptr.end());
    if ((rc = ensure_scratch(ctx, Work::Tables, sizeof(void *) * table.size(), &tab))) return rc;
    if ((rc = upload_small(ctx, tab, table.data(), sizeof(void *) * table.size()))) return rc;   // `table` is a local: pinned ring
    const bool nulls = p->null_policy != POLS_NULL_IGNORE;
    WideArgs a;
    std::memset(&a, 0, sizeof(a));
    Carve cv;
    cv.keep(a.gram, mat * G);
    cv.keep(a.partial, mat * G * (size_t)splits);
    cv.keep(a.coef64, sizeof(double) * G * kt * m);
    if (nulls) {
        cv.keep(a.rowmask, (size_t)b->n_rows);
        cv.keep(a.nfit, sizeof(double) * G);
    }
    if ((rc = carve(ctx, Work::Gram, cv))) return rc;
    if (!st.status) {
        void *sp = nullptr;
        if ((rc = ensure_scratch(ctx, Work::Status, sizeof(int32_t) * G, &sp))) return rc;
        st.status = static_cast<int32_t *>(sp);
    }
    if ((rc = ensure_fallback_epoch(ctx))) return rc;

    a.cols = static_cast<const void *const *>(tab);
    if (m > 1) {
        a.n_targets = m;
        a.ycols = a.cols + b->n_features;
        if (!pptr.empty()) a.pred_cols = static_cast<void *const *>(tab) + b->n_features + m;
    }
    a.y = st.y; a.w = st.w; a.offs = d_offs; a.n_groups = b->n_groups; a.n_rows = b->n_rows;
    a.k_user = b->n_features; a.kt = kt;
    a.splits = (int32_t)splits; a.rows_per_split = rps;
    a.alpha = enet ? p->alpha : plan.ridge_alpha; a.l1_ratio = plan.enet_l1; a.tol = p->tol; a.max_iter = p->max_iter;
    a.positive = p->positive ? 1 : 0; a.active_set = (p->solve_method == POLS_SOLVE_CD_ACTIVE_SET) ? 1 : 0;
    a.pivot_tol = plan.pivot_tol;
    a.rc_factor = plan.rc_factor;
    a.status = st.status; a.fb_flag = ctx->fb_flag; a.epoch = ctx->epoch;
    a.coef = st.coef; a.pred = st.pred; a.resid = st.resid;
    a.null_policy = p->null_policy;
    if (nulls) {
        a.valid = st.valid;
        if ((rc = wide_rowmask_launch(ctx, b->dtype, a))) return rc;
    }
    if ((rc = wide_gram_launch(ctx, b->dtype, a))) return rc;
    if (enet) {
        if ((rc = wide_cd_launch(ctx, b->dtype, a))) return rc;
    } else {
        // (known before the factorisation: wide_chol flags a group with fewer fit rows than columns BY SHAPE under solve_method None / "svd",
        // where the reference picks the SVD without factoring anything, ls.rs:224-231 -- the last pivots of a rank-deficient Gram matrix can
        // come out as positive noise above the threshold)
        a.fix_mode = plan.fix_mode;
        if ((rc = wide_chol_launch(ctx, b->dtype, a))) return rc;
        int workers = (int)std::min<size_t>(G, 64);
        void *wk = nullptr;
        const bool lu = fix_uses_lu(a.fix_mode);
        const int64_t ncmax = lu ? kt : std::min<int64_t>(std::max<int64_t>(1, max_rows), kt);
        a.work_w_elems = (int64_t)(kt + m) * std::max<int64_t>(1, max_rows);
        a.work_stride = a.work_w_elems + ncmax * ncmax + 2 * ncmax + (lu ? (int64_t)kt * m : 0);
        while (workers > 1 && (double)workers * (double)a.work_stride * 8.0 > 1e9) workers /= 2;
        if ((rc = ensure_scratch(ctx, Work::Fixup, sizeof(double) * (size_t)workers * (size_t)a.work_stride, &wk))) return rc;
        a.work = static_cast<double *>(wk);
        if ((rc = wide_minnorm_launch(ctx, b->dtype, a, workers))) return rc;
    }
    if (st.pred || st.resid || a.pred_cols)
        if ((rc = wide_predict_launch(ctx, b->dtype, a))) return rc;
    if (m > 1 && host && pred_cols)
        for (int t = 0; t < m; ++t)
            POLS_HIP(hipMemcpyAsync(pred_cols[t], pptr[t], dtype_size(b->dtype) * (size_t)b->n_rows, hipMemcpyDeviceToHost, ctx->stream));
    if (info) { info->st = st; info->a = a; return POLS_OK; }
    return unstage_outputs(ctx, b, b->n_groups * m, kt, o, st);
}

}  // namespace pols

using namespace pols;

extern "C" {

int pols_least_squares(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, pols_out *o) {
    return ls_core(ctx, b, p, o, nullptr);
}

// ------------------------------------------------------------------ multi-target
int pols_multi_target_least_squares(pols_ctx *ctx, const pols_batch *b, const void *const *y_cols, int32_t n_targets,
                                    const pols_ols_params *p, void *const *pred_cols, void *coef, int32_t *status) {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (!b || !p || !y_cols) return fail(POLS_ERR_INVALID, "batch / params / y_cols is NULL");
    if (n_targets < 1 || n_targets > 256) return fail(POLS_ERR_INVALID, "n_targets must be in 1..256");
    for (int t = 0; t < n_targets; ++t)
        if (!y_cols[t] || (pred_cols && !pred_cols[t])) return fail(POLS_ERR_INVALID, "target / prediction column %d is NULL", t);
    pols_batch bb = *b;
    bb.y = y_cols[0];
    pols_out o;
    std::memset(&o, 0, sizeof(o));
    o.coef = coef; o.status = status;
    if ((rc = check_batch(&bb, &o, K8_KMAX))) return rc;
    if (b->mem == POLS_MEM_DEVICE) {                                 // (the target and prediction columns are read / written 16 bytes at a time like y / pred)
        bool ok = aligned16(b->weights);
        for (int j = 0; j < b->n_features; ++j) ok = ok && aligned16(b->x_cols[j]);
        for (int t = 0; t < n_targets; ++t) ok = ok && aligned16(y_cols[t]) && (!pred_cols || aligned16(pred_cols[t]));
        if (!ok) return fail(POLS_ERR_INVALID, "device columns must be 16-byte aligned");
    }
    // least_squares.py:303-318: unconstrained OLS / ridge only, solve_method in {None, "svd"}
    const double l1 = p->has_l1_ratio ? p->l1_ratio : 0.0;
    if (p->positive || l1 != 0.0)
        return fail(POLS_ERR_PANIC, "Multi-target regression is only supported for unconstrained OLS & Ridge problems.");
    if (!(p->solve_method == POLS_SOLVE_AUTO || p->solve_method == POLS_SOLVE_SVD))
        return fail(POLS_ERR_PANIC, "only solve_method='svd' is supported for multi-target regressions");
    if (!(p->alpha >= 0.0)) return fail(POLS_ERR_PANIC, "alpha must be non-negative");
    if (p->null_policy < POLS_NULL_IGNORE || p->null_policy > POLS_NULL_DROP_WINDOW) return fail(POLS_ERR_INVALID, "unknown null_policy %d", p->null_policy);
    if (b->valid && (p->null_policy == POLS_NULL_IGNORE || p->null_policy == POLS_NULL_ZERO))
        return fail(POLS_ERR_INVALID, "a validity mask needs a drop-family null_policy");
    const int kt = b->n_features + (b->add_intercept ? 1 : 0);
    if (kt + n_targets > K8_KMAX) return fail(POLS_ERR_UNSUPPORTED, "%d columns + %d targets > %d", kt, n_targets, K8_KMAX);
    if (b->n_groups == 0) return POLS_OK;
    // "ignore" is NOT the identity here: the multi-target body builds both arrays with construct_features_array(.., true)
    // (src/expressions.rs:546-547), so nulls the policy leaves in place -- targets included -- are zero-filled: "ignore" == "zero".
    const int policy = p->null_policy == POLS_NULL_IGNORE ? POLS_NULL_ZERO : p->null_policy;
    if (!b->null_free || b->valid) {
        // The plugin body under a null policy (src/expressions.rs:521-591): the joint validity mask over every target (and, unless
        // drop_y_zero_x, every feature), the fit on the rows handle_nulls leaves -- compacted on the device --, then predictions for
        // EVERY row from the zero-filled features, masked under "drop".
        Compacted c;
        if ((rc = compact_nulls(ctx, &bb, policy, &c, y_cols, n_targets))) return rc;
        const bool host = b->mem == POLS_MEM_HOST;
        const size_t G = (size_t)b->n_groups, N = (size_t)b->n_rows, sz = dtype_size(b->dtype);
        const size_t colb = round256(sz * std::max<size_t>(N, 1)), tabb = sizeof(void *) * (size_t)std::max(b->n_features, n_targets);
        void *dcoef = nullptr;
        int32_t *dstat = nullptr;
        char *preds = nullptr;
        MtPredictArgs ma;
        std::memset(&ma, 0, sizeof(ma));
        Carve cv;
        cv.keep(dcoef, sz * G * n_targets * kt);
        cv.keep(dstat, sizeof(int32_t) * G);
        cv.add(ma.xtab, tabb);
        cv.add(ma.ptab, tabb);
        cv.add(preds, host && pred_cols ? colb * (size_t)n_targets : 0);
        if ((rc = carve(ctx, Work::CompactOut, cv))) return rc;
        if (!host && coef) dcoef = coef;
        if (!host && status) dstat = status;
        pols_ols_params pp = *p;
        pp.null_policy = POLS_NULL_IGNORE;
        if ((rc = pols_multi_target_least_squares(ctx, &c.bb, c.ycols.data(), n_targets, &pp, nullptr, dcoef, dstat))) return rc;
        if (pred_cols) {
            // (the inner call uploaded the COMPACTED offsets in place of the frame's: the original ones again)
            const int64_t *d_offs = nullptr;
            int64_t mr = 0;
            if ((rc = upload_offsets(ctx, b->group_offsets, b->n_groups, &d_offs, &mr, b->offsets_generation))) return rc;
            std::vector<void *> pt((size_t)n_targets);
            for (int t = 0; t < n_targets; ++t) pt[(size_t)t] = host ? static_cast<void *>(column(preds, colb, (size_t)t)) : pred_cols[t];
            if ((rc = upload_small(ctx, const_cast<void **>(ma.xtab), c.st.x.data(), sizeof(void *) * (size_t)b->n_features))) return rc;
            if ((rc = upload_small(ctx, const_cast<void **>(ma.ptab), pt.data(), sizeof(void *) * (size_t)n_targets))) return rc;
            ma.w = c.st.w; ma.coef = dcoef; ma.vbytes = c.vbytes; ma.offs = d_offs; ma.n_groups = b->n_groups;
            ma.k_user = b->n_features; ma.kt = kt; ma.m = n_targets;
            ma.mask_drop = p->null_policy == POLS_NULL_DROP ? 1 : 0;                   // ex.rs:575-583
            ma.row_blocks = (int32_t)std::min<int64_t>(1024, std::max<int64_t>(1, (int64_t)(N / std::max<size_t>(G, 1)) / 4096));
            if ((rc = mt_predict_launch(ctx, b->dtype, ma))) return rc;
            if (host)
                for (int t = 0; t < n_targets; ++t)
                    POLS_HIP(hipMemcpyAsync(pred_cols[t], pt[(size_t)t], sz * N, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (host) {
            if (coef) POLS_HIP(hipMemcpyAsync(coef, dcoef, sz * G * n_targets * kt, hipMemcpyDeviceToHost, ctx->stream));
            if (status) POLS_HIP(hipMemcpyAsync(status, dstat, sizeof(int32_t) * G, hipMemcpyDeviceToHost, ctx->stream));
            POLS_HIP(hipStreamSynchronize(ctx->stream));
        }
        return POLS_OK;
    }
    // solve_multi_target (ls.rs:243-260): alpha > 0 -> ridge (SVD form), else minimum-norm least squares: ONE Gram pass over
    // [X | targets] and ONE factorisation serve every target; flagged groups go through the Jacobi pass once as well.
    SolvePlan plan;
    if ((rc = resolve_solve_plan(p, b->dtype, kt, n_targets, &plan))) return rc;
    return wide_static(ctx, &bb, p, &o, kt, plan, y_cols, n_targets, pred_cols);
}

int pols_debug_static_route(const pols_batch *shape, const pols_ols_params *p, const char *const *option_keys,
                            const char *const *option_values, int n_options, char *route_out, int cap) {
    if (!shape || !p || !route_out || cap < 1) return fail(POLS_ERR_INVALID, "NULL argument");
    if (!shape->group_offsets || shape->n_groups < 0) return fail(POLS_ERR_INVALID, "NULL column / offsets pointer");
    Options opt;
    for (int i = 0; i < n_options; ++i)
        if (!options_set(opt, option_keys[i], option_values[i])) return fail(POLS_ERR_INVALID, "unknown option '%s'", option_keys[i] ? option_keys[i] : "");
    int rc, pol = POLS_NULL_IGNORE;
    if ((rc = effective_null_policy(shape, p, &pol))) return rc;
    SolvePlan plan;
    const int kt = shape->n_features + (shape->add_intercept ? 1 : 0);
    if ((rc = resolve_solve_plan(p, shape->dtype, kt, 1, &plan))) return rc;
    OffsetsScan s;
    if (!scan_offsets(shape->group_offsets, shape->n_groups, &s)) return fail(POLS_ERR_INVALID, "group_offsets must be ascending");
    const RoutePick r = pick_static_route(route_inputs(opt, shape, p, pol, plan, s.max_rows, s.aligned, s.hist_cnt, s.hist_rows));
    std::snprintf(route_out, (size_t)cap, "%s", shape->n_groups == 0 ? "none" : route_name(r.route));
    return POLS_OK;
}

}  // extern "C"
