// api_fits.hip -- the per-group fit entries of the C-ABI: pols_ridge_cv (K10), pols_rlm (K11), pols_elastic_net_cv (K12), pols_glm
// (K13), pols_iv2sls (K14), pols_least_squares_absorb (K16), pols_least_squares_absorb2 (K17), pols_glsar (K18), pols_random_effects (K19).  Host code only.  What they share is written once, up front: the opening checks and the staging
// (FitCall), the common fields of the kernel argument structs (fit_frame, fit_segments), the work buffers (Carve, carve), the entry's own
// outputs (ExtraOut), K10's prediction pass (fit_predict), extra input columns (stage_extra_columns), the tile count rlm and glm route by
// (group_tiles) and the stages of the absorb pair.  DESIGN.md, "Adding a per-group fit entry".
#include <algorithm>
#include <cassert>
#include <cmath>

#include "api_internal.hpp"
#include "k10_ridge_path.hpp"
#include "k11_rlm.hpp"
#include "k12_enet_cv.hpp"
#include "k13_glm.hpp"
#include "k14_iv.hpp"
#include "k16_absorb.hpp"
#include "k17_absorb2.hpp"
#include "k18_glsar.hpp"
#include "k19_random_effects.hpp"
#include "k7c_cluster.hpp"
#pragma GCC visibility push(hidden)     // host helpers of this file alone: nothing of them is exported
#include "k17_split.hpp"
#include "k19_split.hpp"
#pragma GCC visibility pop

using namespace pols;

namespace {

// What every entry derives before its own work.
struct FitCall {
    int kt = 0;                      // the frame's columns: n_features + intercept
    int pol = 0;                     // the null policy the kernels see
    bool host = false;
    size_t G = 0, sz = 0;            // groups; bytes per value of the batch dtype
    const int64_t *d_offs = nullptr; // fit_stage: the offsets on the device, the longest group, the columns
    int64_t max_rows = 0;
    Staged st;
};

// The shared checks.  `name` words the messages, `cap` is the entry's limit on the frame's columns (incl. the intercept).
int fit_check(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const void *q, const pols_out *o, const char *name, int cap,
              FitCall *fc) {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if (b && o && b->n_features + (b->add_intercept ? 1 : 0) > cap)
        return fail(POLS_ERR_UNSUPPORTED, "%s: %d features (incl. intercept) > %d", name, b->n_features + (b->add_intercept ? 1 : 0), cap);
    if ((rc = check_batch(b, o, cap))) return rc;
    if (!p || !q) return fail(POLS_ERR_INVALID, "params / %s params is NULL", name);
    if (p->null_policy < POLS_NULL_IGNORE || p->null_policy > POLS_NULL_DROP_WINDOW) return fail(POLS_ERR_INVALID, "unknown null_policy %d", p->null_policy);
    fc->pol = (b->null_free && !b->valid) ? POLS_NULL_IGNORE : p->null_policy;
    if (b->valid && (fc->pol == POLS_NULL_IGNORE || fc->pol == POLS_NULL_ZERO))
        return fail(POLS_ERR_INVALID, "a validity mask needs a drop-family null_policy");
    fc->kt = b->n_features + (b->add_intercept ? 1 : 0);
    fc->host = b->mem == POLS_MEM_HOST;
    fc->G = (size_t)b->n_groups;
    fc->sz = dtype_size(b->dtype);
    return POLS_OK;
}

int fit_stage(pols_ctx *ctx, const pols_batch *b, const pols_out *o, FitCall *fc) {
    int rc = upload_offsets(ctx, b->group_offsets, b->n_groups, &fc->d_offs, &fc->max_rows, b->offsets_generation);
    if (rc) return rc;
    if ((rc = stage_inputs(ctx, b, b->n_groups, fc->kt, o, &fc->st))) return rc;
    return fill_null_weights(ctx, b, &fc->st);
}

// an entry called without its own output struct wants none of its fields
template <typename O> const O *or_none(const O *ro) {
    static const O none = {};
    return ro ? ro : &none;
}

// The fields every argument struct of the family has (templates: the structs stay as the kernels know them).
template <typename A> void fit_frame(A &a, const pols_batch *b, const FitCall &fc) {
    a.y = fc.st.y; a.w = fc.st.w;
    for (int j = 0; j < b->n_features; ++j) a.x[j] = fc.st.x[(size_t)j];
    a.offs = fc.d_offs; a.n_groups = b->n_groups; a.n_rows = b->n_rows;
    a.valid = fc.st.valid; a.null_policy = fc.pol;
    a.k_user = b->n_features; a.kt = fc.kt; a.f32 = b->dtype == POLS_F32 ? 1 : 0;
    a.coef = fc.st.coef; a.status = fc.st.status;
}
template <typename A> void fit_segments(A &a, const SegTables &sg) {
    if (sg.n_seg > 0) { a.seg_offs = sg.offs; a.seg_map = sg.map; a.seg_first = sg.first; a.n_seg = sg.n_seg; }
}

// The entry's own outputs, each registered once: the caller's pointer, the slot of the argument struct, the bytes.  place(): the
// slot of a DEVICE batch is the caller's pointer; the wanted fields of a HOST batch are carved out of `w` (one region each) and
// an unwanted one's slot stays nullptr.  home(): the wanted fields of a HOST batch go home, then the pols_out ones (unstage_outputs).
struct ExtraOut {
    struct Field {
        void *home, *slot, *dev;
        size_t bytes;
        void (*set)(void *slot, void *p);
    };
    static constexpr int CAP = 16;
    Field f[CAP];
    int n = 0;

    template <typename T> void add(T *home, T *&slot, size_t bytes) {
        assert(n < CAP);
        f[n++] = Field{home, &slot, nullptr, bytes, [](void *s, void *p) { *static_cast<T **>(s) = static_cast<T *>(p); }};
    }
    int place(pols_ctx *ctx, const FitCall &fc, Work w) {
        Carve cv;
        for (int i = 0; i < n; ++i) {
            if (!f[i].home) continue;
            f[i].dev = f[i].home;
            if (fc.host) cv.add(f[i].dev, f[i].bytes, &f[i].home);   // (a wanted field of 0 bytes keeps a non-null slot: the kernels tell by it)
        }
        int rc = cv.total() > 0 ? carve(ctx, w, cv) : POLS_OK;
        for (int i = 0; i < n && !rc; ++i)
            if (f[i].home) f[i].set(f[i].slot, f[i].dev);
        return rc;
    }
    int home(pols_ctx *ctx, const pols_batch *b, const pols_out *o, const FitCall &fc) const {
        if (!fc.host) return POLS_OK;
        for (int i = 0; i < n; ++i)
            if (f[i].home && f[i].bytes > 0) POLS_HIP(hipMemcpyAsync(f[i].home, f[i].dev, f[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
        return unstage_outputs(ctx, b, b->n_groups, fc.kt, o, fc.st);
    }
};

// K10's launches over a column list of the caller's: the frame, the columns x[0 .. k_user) and kt coefficients per group.
RidgeCvArgs k10_frame(const pols_batch *b, const FitCall &fc, const SegTables *sg, const void *const *x, int k_user, int kt) {
    RidgeCvArgs a = {};
    a.y = fc.st.y; a.w = fc.st.w;
    for (int j = 0; j < k_user; ++j) a.x[j] = x[j];
    a.offs = fc.d_offs; a.n_groups = b->n_groups; a.n_rows = b->n_rows;
    if (sg) fit_segments(a, *sg);
    a.valid = fc.st.valid; a.null_policy = fc.pol; a.k_user = k_user; a.kt = kt;
    return a;
}

// K10's prediction pass from f64 coefficients (kt per group): pred / resid of the pols_out.  sg: the segment tables, or nullptr.
int fit_predict(pols_ctx *ctx, const pols_batch *b, const FitCall &fc, const SegTables *sg, const void *const *x, int k_user, int kt,
                double *coef64) {
    RidgeCvArgs pa = k10_frame(b, fc, sg, x, k_user, kt);
    pa.coef64 = coef64; pa.pred = fc.st.pred; pa.resid = fc.st.resid;
    return k10_predict_launch(ctx, b->dtype, pa);
}

// n further columns of n_rows batch-dtype values (the GLM offset, the instruments): a HOST batch's are copied into `w`, a DEVICE
// batch's are taken where they are.
int stage_extra_columns(pols_ctx *ctx, const pols_batch *b, Work w, const void *const *src, int n, const void **dst) {
    const size_t bytes = dtype_size(b->dtype) * (size_t)b->n_rows;
    const bool copy = b->mem == POLS_MEM_HOST && bytes > 0 && n > 0;
    Carve cv;
    for (int j = 0; j < n; ++j) {
        dst[j] = src[j];
        if (copy) cv.add(dst[j], bytes);
    }
    int rc = copy ? carve(ctx, w, cv) : POLS_OK;
    if (rc) return rc;
    for (int j = 0; j < n; ++j) {
        if (copy) POLS_HIP(hipMemcpyAsync(const_cast<void *>(dst[j]), src[j], bytes, hipMemcpyHostToDevice, ctx->stream));
        else if (b->mem == POLS_MEM_DEVICE && !aligned16(src[j])) return fail(POLS_ERR_INVALID, "device columns must be 16-byte aligned");
    }
    return POLS_OK;
}

// What rlm and glm route by: the tiles group g spans from the 16-byte grid point at or below its first row.
int group_tiles(const pols_batch *b, int64_t g, int64_t *tiles) {
    const int64_t s = b->group_offsets[g], e = b->group_offsets[g + 1], vec = b->dtype == POLS_F32 ? 4 : 2;
    if (e < s) return fail(POLS_ERR_INVALID, "group_offsets must not decrease");
    *tiles = e > s ? (e - (s & ~(vec - 1)) + 255) / 256 : 0;
    return POLS_OK;
}

// ---------------------------------------------------------------- the stages of the absorb pair (K16, K17)
// The checks behind fit_check, in the order they fire.  `name` words the messages; `iter`: K17's stop rule (K16: nullptr); fe / fe2: the
// entry's effect columns (a frame without groups is not held to the alignment rule: the entry returns before any work).
int absorb_check(const pols_batch *b, const pols_ols_params *p, const pols_out *o, const FitCall &fc, const char *name,
                 const int64_t *const *ids, int n_ids, int cov_type, const pols_absorb2_params *iter, const void *fe, const void *fe2) {
    if (p->alpha != 0.0 || p->positive || (p->has_l1_ratio && p->l1_ratio > 0.0))
        return fail(POLS_ERR_INVALID, "%s: alpha / positive / l1_ratio do not apply (penalised absorbed fits are not built)", name);
    if (b->n_features < 1) return fail(POLS_ERR_INVALID, "%s: no feature column", name);
    for (int w = 0; w < n_ids; ++w)
        if (!ids[w]) return fail(POLS_ERR_INVALID, "%s: %s is NULL", name, n_ids == 2 ? "ids / ids2" : "ids");
    if (cov_type != POLS_COV_NONROBUST && cov_type != POLS_COV_CLUSTER)
        return fail(POLS_ERR_INVALID, "%s: cov_type %d is not NONROBUST / CLUSTER", name, cov_type);
    if (iter && iter->max_iter < 1) return fail(POLS_ERR_INVALID, "%s: max_iter %d < 1", name, iter->max_iter);
    if (iter && (!(iter->tol > 0.0) || !std::isfinite(iter->tol))) return fail(POLS_ERR_INVALID, "%s: tol %g is not positive and finite", name, iter->tol);
    if (b->n_rows >= ((int64_t)1 << 31)) return fail(POLS_ERR_UNSUPPORTED, "%s: %lld rows >= 2^31", name, (long long)b->n_rows);
    // (pred / resid / fe / fe1 are written 16 bytes at a time; fe2 goes out row by row and is held to the same rule as its sibling)
    if (b->n_groups > 0 && !fc.host && !(aligned16(fe) && aligned16(fe2) && aligned16(o->pred) && aligned16(o->resid)))
        return fail(POLS_ERR_INVALID, "device columns must be 16-byte aligned");
    return POLS_OK;
}

// The id columns on the device: a HOST batch's are copied into `w` (one region each), a DEVICE batch's are taken in place.
int stage_ids(pols_ctx *ctx, const FitCall &fc, Work w, const int64_t *const *ids, int n, size_t N, const int64_t **d_ids) {
    Carve cv;
    for (int j = 0; j < n; ++j) {
        d_ids[j] = ids[j];
        if (fc.host) cv.add(d_ids[j], sizeof(int64_t) * N + 8);
    }
    int rc = fc.host ? carve(ctx, w, cv) : POLS_OK;
    if (rc) return rc;
    for (int j = 0; j < n; ++j)
        if (fc.host && N > 0) POLS_HIP(hipMemcpyAsync(const_cast<int64_t *>(d_ids[j]), ids[j], sizeof(int64_t) * N, hipMemcpyHostToDevice, ctx->stream));
    return POLS_OK;
}

// The categories of n id columns (c[j]: the frame, .ids and .order are set): the count / first / index tables of each in `w`, K16's count
// launch and the copy of the number of categories into c[j].n_cats -- which holds once the CALLER has synchronised the stream.
int categories(pols_ctx *ctx, Work w, AbsorbArgs *c, int n, size_t items, size_t N) {
    Carve cv;
    for (int j = 0; j < n; ++j) {
        cv.add(c[j].item_cnt, sizeof(int32_t) * items); cv.add(c[j].item_first, sizeof(int64_t) * (items + 1));
        cv.add(c[j].catidx, sizeof(int32_t) * N + 4);
    }
    int rc = carve(ctx, w, cv);
    if (rc) return rc;
    for (int j = 0; j < n; ++j) {
        if ((rc = k16_count_launch(ctx, c[j]))) return rc;
        POLS_HIP(hipMemcpyAsync(&c[j].n_cats, c[j].item_first + items, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    return POLS_OK;
}

// The statistics both entries return, and whether any is wanted: only then the residual pass and the finish run.  (The entry's own
// fields follow in the order of its struct: the order of registration is the order of a HOST batch's carve.)
template <typename A, typename O> bool absorb_stats_out(ExtraOut &xo, A &a, const O *ro, size_t G, int kc) {
    xo.add(ro->se, a.se, sizeof(double) * G * kc); xo.add(ro->t_values, a.t_values, sizeof(double) * G * kc);
    xo.add(ro->p_values, a.p_values, sizeof(double) * G * kc); xo.add(ro->sigma2, a.sigma2, sizeof(double) * G);
    xo.add(ro->r2_within, a.r2_within, sizeof(double) * G); xo.add(ro->r2, a.r2, sizeof(double) * G);
    return ro->se || ro->t_values || ro->p_values || ro->sigma2 || ro->r2_within || ro->r2;
}

// K17: the two orders (K7c's builder keeps one at a time, so the first is copied before the builder runs again) and, behind them, the
// group list of a mixed frame.
int absorb2_orders(pols_ctx *ctx, const pols_batch *b, const FitCall &fc, const int64_t *const *d_ids, const K17Split &sp, Absorb2Args &a,
                   const int32_t **d_list) {
    const size_t N = (size_t)b->n_rows, ib = sizeof(uint32_t) * N + 4;
    uint32_t *ord1 = nullptr;
    int32_t *list = nullptr;
    Carve cv;
    cv.add(ord1, ib); cv.add(a.pos1, ib); cv.add(a.perm2, ib);
    cv.add(list, sp.mixed() ? sizeof(int32_t) * fc.G : 0);
    int rc = carve(ctx, Work::Absorb2Order, cv);
    if (rc) return rc;
    if (sp.mixed() && (rc = upload_small(ctx, list, sp.list.data(), sizeof(int32_t) * fc.G))) return rc;
    *d_list = list;
    if ((rc = k7c_order_launch(ctx, d_ids[0], fc.d_offs, b->n_groups, b->n_rows, &a.order1))) return rc;
    if (a.order1) {
        POLS_HIP(hipMemcpyAsync(ord1, a.order1, sizeof(uint32_t) * N, hipMemcpyDeviceToDevice, ctx->stream));
        a.order1 = ord1;
    }
    return k7c_order_launch(ctx, d_ids[1], fc.d_offs, b->n_groups, b->n_rows, &a.order2);
}

// K17: what the numbers of categories size (per id column: the starts, the means and their weight sums -- the same bytes twice --, the
// weights, effects and labels), the staged columns and the moments.
int absorb2_tables(pols_ctx *ctx, Absorb2Args &a, AbsorbArgs *way, size_t items, size_t G, size_t N, int k, bool cluster) {
    const size_t nc1 = (size_t)way[0].n_cats, nc2 = (size_t)way[1].n_cats, kz = (size_t)k + 1;
    const size_t am1b = sizeof(double) * kz * nc1 + 8, am2b = sizeof(double) * kz * nc2 + 8, d1b = sizeof(double) * nc1 + 8, d2b = sizeof(double) * nc2 + 8;
    Carve cats, cols, moments;
    cats.add(way[0].cat_start, sizeof(int64_t) * (nc1 + 1)); cats.add(way[1].cat_start, sizeof(int64_t) * (nc2 + 1));
    cats.add(a.am1, am1b); cats.add(a.am2, am2b);
    cats.add(a.aw1, am1b); cats.add(a.aw2, am2b);
    cats.add(a.wc1, d1b); cats.add(a.eff1, d1b);
    cats.add(a.wc2, d2b); cats.add(a.eff2, d2b);
    cats.add(a.lab1, sizeof(int32_t) * nc1 + 4); cats.add(a.lab2, sizeof(int32_t) * nc2 + 4);
    cats.add(a.resid_part, sizeof(double) * nc1 * k17_resid_stride(k, cluster) + 8);
    cols.add(a.cols, sizeof(double) * kz * N + 8); cols.add(a.wfit, sizeof(double) * N + 8);
    cols.add(a.rowlab, sizeof(int32_t) * N + 4); cols.add(a.fitb, N + 1);
    moments.add(a.gram_part, sizeof(double) * items * k17_gram_stride(k)); moments.add(a.state, sizeof(double) * G * k17_state_stride(k));
    moments.add(a.colstat, sizeof(double) * G * kz * K17_COLSTAT); moments.add(a.grpstat, sizeof(double) * G * K17_GRPSTAT);
    int rc = carve(ctx, Work::Absorb2Cats, cats);
    if (!rc) rc = carve(ctx, Work::Absorb2Cols, cols);
    return rc ? rc : carve(ctx, Work::Absorb2Moments, moments);
}

// K17: the launches behind the tables -- stage, demean (resident, global, or one of each over the two halves of a mixed frame's list),
// moments, solve, the residual pass and the finish when a wanted output needs a residual, the prediction pass.
int absorb2_launches(pols_ctx *ctx, int dtype, const Absorb2Args &a, const K17Split &sp, const int32_t *d_list, bool need_rows) {
    int rc = k17_stage_launch(ctx, dtype, a);
    if (rc) return rc;
    if (sp.mixed()) {
        Absorb2Args part = a;
        part.list = d_list; part.n_list = sp.n_res;
        if ((rc = k17_demean_launch(ctx, part, true, sp.max_res))) return rc;
        part.list = d_list + sp.n_res; part.n_list = a.n_groups - sp.n_res;
        if ((rc = k17_demean_launch(ctx, part, false, sp.max_glb))) return rc;
    } else if ((rc = k17_demean_launch(ctx, a, sp.n_res > 0, sp.n_res > 0 ? sp.max_res : sp.max_glb))) return rc;
    if ((rc = k17_gram_launch(ctx, a))) return rc;
    if ((rc = k17_solve_launch(ctx, a))) return rc;
    if (need_rows) {
        if ((rc = k17_resid_launch(ctx, a))) return rc;
        if ((rc = k17_finish_launch(ctx, a))) return rc;
    }
    return k17_predict_launch(ctx, dtype, a);
}

}  // namespace

extern "C" {

void pols_ridge_cv_params_default(pols_ridge_cv_params *q) {
    if (!q) return;
    q->alphas = nullptr;
    q->n_alphas = 0;
}

// K10 (k10_ridge_path.hip): Gram pass, eigendecomposition, row pass over the candidates, pick, prediction pass with the winner's
// coefficients.  Null policies are fused into the tile staging and into the prediction pass, as in ls_core's streamed path.
int pols_ridge_cv(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_ridge_cv_params *q, pols_out *o,
                  const pols_ridge_cv_out *ro) {
    FitCall fc;
    int rc = fit_check(ctx, b, p, q, o, "ridge_cv", K10_KMAX, &fc);
    if (rc) return rc;
    if (!q->alphas || q->n_alphas < 1) return fail(POLS_ERR_INVALID, "ridge_cv: the grid of candidates is empty");
    if (q->n_alphas > K10_MAX_ALPHAS) return fail(POLS_ERR_UNSUPPORTED, "ridge_cv: %d candidates > %d", q->n_alphas, K10_MAX_ALPHAS);
    for (int j = 0; j < q->n_alphas; ++j)
        if (!(q->alphas[j] >= 0.0) || !std::isfinite(q->alphas[j])) return fail(POLS_ERR_INVALID, "ridge_cv: candidate %d is negative or not finite", j);
    if (p->positive || (p->has_l1_ratio && p->l1_ratio > 0.0))
        return fail(POLS_ERR_INVALID, "ridge_cv: positive / l1_ratio fits have no hat matrix");
    if (b->n_groups == 0) return POLS_OK;
    ro = or_none(ro);
    if ((rc = fit_stage(ctx, b, o, &fc))) return rc;
    const int kt = fc.kt, na = q->n_alphas;
    const size_t G = fc.G;
    SegTables sg;
    if ((rc = ensure_segments(ctx, b, fc.max_rows, 0, &sg))) return rc;
    const size_t items = sg.n_seg > 0 ? (size_t)sg.n_seg : G;
    RidgeCvArgs a = {};
    fit_frame(a, b, fc);
    fit_segments(a, sg);
    a.n_alphas = na;
    Carve gram, scores;
    gram.add(a.gram_part, sizeof(double) * items * k10_gram_stride(kt)); gram.add(a.eig, sizeof(double) * G * k10_eig_stride(kt));
    scores.add(a.alphas, sizeof(double) * (size_t)na); scores.add(a.score_part, sizeof(double) * items * (size_t)na);
    scores.add(a.coef64, sizeof(double) * G * kt);
    if ((rc = carve(ctx, Work::RidgeCvGram, gram))) return rc;
    if ((rc = carve(ctx, Work::RidgeCvScores, scores))) return rc;
    if ((rc = upload_small(ctx, const_cast<double *>(a.alphas), q->alphas, sizeof(double) * (size_t)na))) return rc;
    ExtraOut xo;
    xo.add(ro->alpha, a.alpha, sizeof(double) * G);
    xo.add(ro->score, a.score, sizeof(double) * G);
    xo.add(ro->alpha_index, a.alpha_index, sizeof(int32_t) * G);
    xo.add(ro->cv_scores, a.cv_scores, sizeof(double) * G * (size_t)na);
    xo.add(ro->coef_path, a.coef_path, fc.sz * G * (size_t)na * kt);
    if ((rc = xo.place(ctx, fc, Work::RidgeCvOut))) return rc;
    ctx->last_kernel = sg.n_seg > 0 ? "k10_ridge_path_split" : "k10_ridge_path";
    if ((rc = k10_gram_launch(ctx, b->dtype, a))) return rc;
    if ((rc = k10_eig_launch(ctx, a))) return rc;
    if ((rc = k10_rows_launch(ctx, b->dtype, a))) return rc;
    if ((rc = k10_pick_launch(ctx, a))) return rc;
    a.pred = fc.st.pred; a.resid = fc.st.resid;
    if ((rc = k10_predict_launch(ctx, b->dtype, a))) return rc;
    return xo.home(ctx, b, o, fc);
}

void pols_rlm_params_default(pols_rlm_params *q) {
    if (!q) return;
    q->norm = POLS_RLM_HUBER;
    q->c = 0.0;
    q->max_iter = 50;
    q->tol = 1e-8;
}

// K11 (k11_rlm.hip): the whole iteration of a group in one workgroup -- one launch for the groups that stay resident in LDS, one for
// those that are streamed -- then K10's prediction pass with the f64 coefficients.
int pols_rlm(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_rlm_params *q, pols_out *o, const pols_rlm_out *ro) {
    FitCall fc;
    int rc = fit_check(ctx, b, p, q, o, "rlm", K11_KMAX, &fc);
    if (rc) return rc;
    if (p->alpha != 0.0 || p->positive || (p->has_l1_ratio && p->l1_ratio > 0.0))
        return fail(POLS_ERR_INVALID, "rlm: alpha / positive / l1_ratio do not apply to the M-estimator");
    if (q->norm != POLS_RLM_HUBER && q->norm != POLS_RLM_BISQUARE) return fail(POLS_ERR_INVALID, "rlm: unknown norm %d", q->norm);
    if (!std::isfinite(q->c)) return fail(POLS_ERR_INVALID, "rlm: c is not finite");
    if (q->max_iter < 1) return fail(POLS_ERR_INVALID, "rlm: max_iter %d < 1", q->max_iter);
    if (!(q->tol > 0.0) || !std::isfinite(q->tol)) return fail(POLS_ERR_INVALID, "rlm: tol %g is not positive and finite", q->tol);
    if (b->n_groups == 0) return POLS_OK;
    ro = or_none(ro);
    if (!fc.host && !aligned16(ro->weights)) return fail(POLS_ERR_INVALID, "device columns must be 16-byte aligned");   // (written 16 bytes at a time)
    const int kt = fc.kt;
    const size_t G = fc.G;
    // which form serves which group
    const int cap = ctx->opt.rlm_engine == 1 ? -1 : k11_resident_tiles(kt);
    int64_t n_res = 0, n_str = 0, res_tiles = 0, str_rows = 0, tiles = 0;
    for (int64_t g = 0; g < b->n_groups; ++g) {
        if ((rc = group_tiles(b, g, &tiles))) return rc;
        if (tiles <= cap) { ++n_res; res_tiles = std::max(res_tiles, tiles); }
        else { ++n_str; str_rows = std::max(str_rows, b->group_offsets[g + 1] - b->group_offsets[g]); }
    }
    if (str_rows > K11_STREAM_MAX_ROWS)
        return fail(POLS_ERR_UNSUPPORTED, "rlm: a group of %lld rows > %lld (one workgroup walks a streamed group; the split form is not built)",
                    (long long)str_rows, (long long)K11_STREAM_MAX_ROWS);
    if ((rc = fit_stage(ctx, b, o, &fc))) return rc;
    RlmArgs a = {};
    fit_frame(a, b, fc);
    a.norm = q->norm; a.max_iter = q->max_iter; a.tol = q->tol;
    a.c = q->c > 0.0 ? q->c : (q->norm == POLS_RLM_HUBER ? 1.345 : 4.685);
    a.res_tiles = cap; a.ts = (int32_t)res_tiles * 256 + 1;
    Carve coef, rows;
    coef.add(a.coef64, sizeof(double) * G * kt);
    rows.add(a.rows, sizeof(double) * (size_t)b->n_rows);          // (stays nullptr unless a group is streamed)
    if ((rc = carve(ctx, Work::RlmCoef, coef))) return rc;
    if (n_str > 0 && (rc = carve(ctx, Work::RlmRows, rows))) return rc;
    ExtraOut xo;
    xo.add(ro->scale, a.scale, sizeof(double) * G);
    xo.add(ro->n_iter, a.n_iter, sizeof(int32_t) * G);
    xo.add(ro->weights, a.weights, fc.sz * (size_t)b->n_rows);
    if ((rc = xo.place(ctx, fc, Work::RlmOut))) return rc;
    ctx->last_kernel = n_res >= n_str ? "k11_rlm_resident" : "k11_rlm_stream";
    if (n_res > 0 && (rc = k11_rlm_launch(ctx, b->dtype, a, true))) return rc;
    if (n_str > 0 && (rc = k11_rlm_launch(ctx, b->dtype, a, false))) return rc;
    if ((rc = fit_predict(ctx, b, fc, nullptr, a.x, a.k_user, kt, a.coef64))) return rc;
    return xo.home(ctx, b, o, fc);
}

long long pols_glm_resident_lds(int kt, int cols, int elem, int tiles) { return (long long)k13_resident_lds(kt, cols, (size_t)elem, tiles); }
int pols_glm_resident_tiles(int kt, int cols, int elem, int per_cu) { return k13_resident_tiles(kt, cols, (size_t)elem, per_cu); }

void pols_glm_params_default(pols_glm_params *q) {
    if (!q) return;
    q->family = POLS_GLM_BINOMIAL;
    q->max_iter = 25;
    q->tol = 1e-8;
    q->offset = nullptr;
}

// K13 (k13_glm.hip): the groups that stay resident in LDS iterate in one launch; the others are cut into segments and iterate with a
// segment pass and a per-group pass per update, until the device counter of iterating groups reads zero; then K13's prediction pass
// with the f64 coefficients.
int pols_glm(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_glm_params *q, pols_out *o, const pols_glm_out *ro) {
    FitCall fc;
    int rc = fit_check(ctx, b, p, q, o, "glm", K13_KMAX, &fc);
    if (rc) return rc;
    if (p->alpha != 0.0 || p->positive || (p->has_l1_ratio && p->l1_ratio > 0.0))
        return fail(POLS_ERR_INVALID, "glm: alpha / positive / l1_ratio do not apply (penalised GLMs are not built)");
    if (q->family != POLS_GLM_BINOMIAL && q->family != POLS_GLM_POISSON) return fail(POLS_ERR_INVALID, "glm: unknown family %d", q->family);
    if (q->max_iter < 1) return fail(POLS_ERR_INVALID, "glm: max_iter %d < 1", q->max_iter);
    if (!(q->tol > 0.0) || !std::isfinite(q->tol)) return fail(POLS_ERR_INVALID, "glm: tol %g is not positive and finite", q->tol);
    if (b->n_groups == 0) return POLS_OK;
    ro = or_none(ro);
    const int kt = fc.kt;
    const size_t G = fc.G, sz = fc.sz;
    // which form serves which group
    const int cols = b->n_features + 1 + (b->weights ? 1 : 0) + (q->offset ? 1 : 0);
    // (two resident launches: the groups whose LDS request leaves room for a second workgroup on a CU, and the longer ones -- one long
    //  group must not size the request of a whole frame of short ones)
    const int cap = ctx->opt.glm_engine == 1 ? -1 : k13_resident_tiles(kt, cols, sz, 1);
    const int cap2 = std::min(cap, k13_resident_tiles(kt, cols, sz, 2));
    int64_t n_res = 0, n_spl = 0, res_tiles = 0, res2_tiles = 0, n_res1 = 0, tiles = 0;
    for (int64_t g = 0; g < b->n_groups; ++g) {
        if ((rc = group_tiles(b, g, &tiles))) return rc;
        if (tiles <= cap2) { ++n_res; res2_tiles = std::max(res2_tiles, tiles); }
        else if (tiles <= cap) { ++n_res; ++n_res1; res_tiles = std::max(res_tiles, tiles); }
        else ++n_spl;
    }
    if ((rc = fit_stage(ctx, b, o, &fc))) return rc;
    const void *d_off = nullptr;
    if ((rc = stage_extra_columns(ctx, b, Work::GlmOffset, &q->offset, q->offset ? 1 : 0, &d_off))) return rc;
    if (!fc.host && !aligned16(ro->linpred)) return fail(POLS_ERR_INVALID, "device columns must be 16-byte aligned");
    SegTables sg;
    if (n_spl > 0 && (rc = ensure_segments(ctx, b, fc.max_rows, sizeof(double) * k13_part_stride(kt), &sg))) return rc;
    GlmArgs a = {};
    fit_frame(a, b, fc);
    fit_segments(a, sg);
    a.o = d_off;
    a.family = q->family; a.max_iter = q->max_iter; a.tol = q->tol;
    a.res_tiles = cap;
    double *seg_part = reinterpret_cast<double *>(sg.extra);       // (the partial sums of a split frame lie behind its segment tables)
    Carve coef, state;
    coef.add(a.coef64, sizeof(double) * G * kt);
    state.add(a.active, 256); state.add(a.state, sizeof(double) * G * k13_state_stride(kt));
    state.add(a.part, sg.n_seg > 0 ? 0 : sizeof(double) * G * k13_part_stride(kt), &seg_part);
    if ((rc = carve(ctx, Work::GlmCoef, coef))) return rc;
    if (n_spl > 0 && (rc = carve(ctx, Work::GlmState, state))) return rc;
    ExtraOut xo;
    xo.add(ro->deviance, a.deviance, sizeof(double) * G);
    xo.add(ro->se, a.se, sizeof(double) * G * kt);
    xo.add(ro->n_iter, a.n_iter, sizeof(int32_t) * G);
    xo.add(ro->linpred, a.linpred, sz * (size_t)b->n_rows);
    if ((rc = xo.place(ctx, fc, Work::GlmOut))) return rc;
    ctx->last_kernel = n_res >= n_spl ? "k13_glm_resident" : "k13_glm_split";
    if (n_res > n_res1) {
        a.res_from = -1; a.res_to = cap2; a.ts = (int32_t)res2_tiles * 256 + 1;
        if ((rc = k13_resident_launch(ctx, b->dtype, a))) return rc;
    }
    if (n_res1 > 0) {
        a.res_from = cap2; a.res_to = cap; a.ts = (int32_t)res_tiles * 256 + 1;
        if ((rc = k13_resident_launch(ctx, b->dtype, a))) return rc;
    }
    if (n_spl > 0) {
        const int32_t n_active = (int32_t)std::min<int64_t>(n_spl, 0x7fffffff);
        if ((rc = upload_small(ctx, a.active, &n_active, sizeof(n_active)))) return rc;
        // one update per turn: at most max_iter updates and the start, then every group has stopped
        for (int turn = 0; turn <= q->max_iter; ++turn) {
            if ((rc = k13_split_launch(ctx, b->dtype, a, turn == 0))) return rc;
            int32_t left = 0;
            POLS_HIP(hipMemcpyAsync(&left, a.active, sizeof(left), hipMemcpyDeviceToHost, ctx->stream));
            POLS_HIP(hipStreamSynchronize(ctx->stream));           // the host decides whether another update is launched
            if (left <= 0) break;
        }
    }
    a.pred = fc.st.pred; a.resid = fc.st.resid;
    if ((rc = k13_predict_launch(ctx, b->dtype, a))) return rc;
    return xo.home(ctx, b, o, fc);
}

void pols_iv_params_default(pols_iv_params *q) {
    if (!q) return;
    q->n_endog = 0;
    q->z_cols = nullptr;
    q->n_instruments = 0;
    q->cov_type = POLS_COV_NONROBUST;
    q->small_sample = 1;
}

// K14 (k14_iv.hip): K10's Gram launch over the concatenated columns [X1 | X2 | Z2], the per-group solve, the row pass for RSS and the
// robust meat (only when a wanted output needs it), the per-group finish, then K10's prediction pass with the f64 coefficients.
int pols_iv2sls(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_iv_params *q, pols_out *o, const pols_iv_out *ro) {
    FitCall fc;
    int rc = fit_check(ctx, b, p, q, o, "iv", K14_TMAX, &fc);
    if (rc) return rc;
    if (p->alpha != 0.0 || p->positive || (p->has_l1_ratio && p->l1_ratio > 0.0))
        return fail(POLS_ERR_INVALID, "iv2sls: alpha / positive / l1_ratio do not apply");
    if (q->n_endog < 1 || q->n_endog > b->n_features) return fail(POLS_ERR_INVALID, "iv2sls: n_endog %d outside 1..%d", q->n_endog, b->n_features);
    if (q->n_instruments < q->n_endog) return fail(POLS_ERR_INVALID, "iv2sls: %d instruments < %d endogenous regressors", q->n_instruments, q->n_endog);
    if (!q->z_cols) return fail(POLS_ERR_INVALID, "iv2sls: z_cols is NULL");
    for (int j = 0; j < q->n_instruments; ++j)
        if (!q->z_cols[j] && b->n_rows) return fail(POLS_ERR_INVALID, "iv2sls: z_cols[%d] is NULL", j);
    if (q->cov_type != POLS_COV_NONROBUST && q->cov_type != POLS_COV_HC0 && q->cov_type != POLS_COV_HC1)
        return fail(POLS_ERR_INVALID, "iv2sls: cov_type %d is not NONROBUST / HC0 / HC1", q->cov_type);
    // the frame's columns are the regressors (fc.kt = kx: what is staged and what coef holds); the cap counts the instruments too
    const int nf = b->n_features, m = q->n_instruments, icpt = b->add_intercept ? 1 : 0, kx = fc.kt, T = kx + m, L = kx - q->n_endog + m;
    if (T > K14_TMAX) return fail(POLS_ERR_UNSUPPORTED, "iv2sls: %d regressors (incl. intercept) + %d instruments > %d", kx, m, K14_TMAX);
    if (b->n_groups == 0) return POLS_OK;
    ro = or_none(ro);
    const int pol = fc.pol;
    const bool robust = q->cov_type != POLS_COV_NONROBUST;
    const bool need_rows = ro->se || ro->t_values || ro->p_values || ro->cov || ro->sigma2 || ro->sargan || ro->sargan_p;
    const size_t G = fc.G;
    if ((rc = fit_stage(ctx, b, o, &fc))) return rc;
    IvArgs a = {};
    fit_frame(a, b, fc);
    if ((rc = stage_extra_columns(ctx, b, Work::IvInputs, q->z_cols, m, a.x + nf))) return rc;
    SegTables sg;
    if ((rc = ensure_segments(ctx, b, fc.max_rows, 0, &sg))) return rc;
    fit_segments(a, sg);
    const size_t items = sg.n_seg > 0 ? (size_t)sg.n_seg : G;
    const bool pred_all = pol == POLS_NULL_DROP && (fc.st.pred || fc.st.resid);   // the one policy whose prediction pass masks rows
    Carve moments, state;
    moments.add(a.gram_part, sizeof(double) * items * k10_gram_stride(T)); moments.add(a.rows_part, sizeof(double) * items * k14_rows_stride(kx, robust));
    state.add(a.state, sizeof(double) * G * k14_state_stride(kx, L)); state.add(a.coefp, sizeof(double) * G * (size_t)(pred_all ? T : kx));
    if ((rc = carve(ctx, Work::IvMoments, moments))) return rc;
    if ((rc = carve(ctx, Work::IvState, state))) return rc;
    a.k_user = nf + m; a.kt = T;                               // of the staged list [X1 | X2 | Z2]
    a.n_feat = nf; a.n_endog = q->n_endog; a.n_inst = m; a.icpt = icpt;
    a.cov_type = q->cov_type; a.small_sample = q->small_sample ? 1 : 0; a.pred_all = pred_all ? 1 : 0;
    ExtraOut xo;
    xo.add(ro->se, a.se, sizeof(double) * G * kx);
    xo.add(ro->t_values, a.t_values, sizeof(double) * G * kx);
    xo.add(ro->p_values, a.p_values, sizeof(double) * G * kx);
    xo.add(ro->cov, a.cov, sizeof(double) * G * kx * kx);
    xo.add(ro->sigma2, a.sigma2, sizeof(double) * G);
    xo.add(ro->sargan, a.sargan, sizeof(double) * G);
    xo.add(ro->sargan_p, a.sargan_p, sizeof(double) * G);
    xo.add(ro->first_stage_f, a.first_stage_f, sizeof(double) * G * (size_t)q->n_endog);
    xo.add(ro->partial_r2, a.partial_r2, sizeof(double) * G * (size_t)q->n_endog);
    xo.add(ro->n_obs, a.n_obs, sizeof(int64_t) * G);
    if ((rc = xo.place(ctx, fc, Work::IvOut))) return rc;
    ctx->last_kernel = sg.n_seg > 0 ? "k14_iv2sls_split" : "k14_iv2sls";
    RidgeCvArgs ga = k10_frame(b, fc, &sg, a.x, nf + m, T);    // K10's Gram launch over the whole list
    ga.gram_part = const_cast<double *>(a.gram_part);
    if ((rc = k10_gram_launch(ctx, b->dtype, ga))) return rc;
    if ((rc = k14_solve_launch(ctx, a))) return rc;
    if (need_rows) {
        // the plain RSS needs the regressors and y alone: the instruments are staged only where the robust meat reads them or their nulls drop rows
        IvArgs ra = a;
        const bool z_drops = pol == POLS_NULL_DROP || pol == POLS_NULL_DROP_ZERO || pol == POLS_NULL_DROP_WINDOW;
        if (!robust && !z_drops) { ra.k_user = nf; ra.kt = kx; }
        if ((rc = k14_rows_launch(ctx, b->dtype, ra))) return rc;
        if ((rc = k14_finish_launch(ctx, a))) return rc;
    }
    // the prediction pass: the regressors alone, or -- "drop" -- the whole list with zero coefficients for the instruments, whose nulls mask rows
    if ((rc = fit_predict(ctx, b, fc, &sg, a.x, pred_all ? nf + m : nf, pred_all ? T : kx, a.coefp))) return rc;
    return xo.home(ctx, b, o, fc);
}

void pols_glsar_params_default(pols_glsar_params *q) {
    if (!q) return;
    q->method = POLS_AR1_PRAIS_WINSTEN;
    q->max_iter = 100;
    q->tol = 1e-6;
}

// K18 (k18_glsar.hip): the lag-Gram launch (S, the lag-one cross-moments C and the row count per item: the columns are read once),
// the per-group solve with the whole iteration, the row pass and the per-group finish (only when a wanted output needs a residual),
// then K10's prediction pass with the f64 coefficients.
int pols_glsar(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_glsar_params *q, pols_out *o, const pols_glsar_out *ro) {
    FitCall fc;
    int rc = fit_check(ctx, b, p, q, o, "glsar", K18_KMAX, &fc);
    if (rc) return rc;
    if (p->alpha != 0.0 || p->positive || (p->has_l1_ratio && p->l1_ratio > 0.0))
        return fail(POLS_ERR_INVALID, "glsar: alpha / positive / l1_ratio do not apply");
    if (q->method != POLS_AR1_COCHRANE_ORCUTT && q->method != POLS_AR1_PRAIS_WINSTEN) return fail(POLS_ERR_INVALID, "glsar: unknown method %d", q->method);
    if (q->max_iter < 1) return fail(POLS_ERR_INVALID, "glsar: max_iter %d < 1", q->max_iter);
    if (!(q->tol > 0.0) || !std::isfinite(q->tol)) return fail(POLS_ERR_INVALID, "glsar: tol %g is not positive and finite", q->tol);
    if (fc.kt < 1) return fail(POLS_ERR_INVALID, "glsar: no column");
    // the lag partner of a row is the row before it: a policy that takes rows out of the fit needs an in-tile scan, weights a second scaling
    if (fc.pol != POLS_NULL_IGNORE && fc.pol != POLS_NULL_ZERO)
        return fail(POLS_ERR_UNSUPPORTED, "glsar: drop-family null policies are not built (pass null_free data, \"ignore\" or \"zero\")");
    if (b->weights) return fail(POLS_ERR_UNSUPPORTED, "glsar: weights are not built");
    if (b->n_groups == 0) return POLS_OK;
    ro = or_none(ro);
    const bool need_rows = ro->se || ro->t_values || ro->p_values || ro->cov || ro->sigma2 || ro->dw || ro->dw_ols;
    const int kt = fc.kt;
    const size_t G = fc.G;
    if ((rc = fit_stage(ctx, b, o, &fc))) return rc;
    SegTables sg;
    if ((rc = ensure_segments(ctx, b, fc.max_rows, 0, &sg))) return rc;
    const size_t items = sg.n_seg > 0 ? (size_t)sg.n_seg : G;
    GlsarArgs a = {};
    fit_frame(a, b, fc);
    fit_segments(a, sg);
    a.method = q->method; a.max_iter = q->max_iter; a.tol = q->tol;
    Carve moments, state;
    moments.add(a.gram_part, sizeof(double) * items * k18_gram_stride(kt)); moments.add(a.rows_part, sizeof(double) * items * K18_ROWS_STRIDE);
    state.add(a.state, sizeof(double) * G * k18_state_stride(kt)); state.add(a.coefp, sizeof(double) * G * (size_t)kt);
    if ((rc = carve(ctx, Work::GlsarMoments, moments))) return rc;
    if ((rc = carve(ctx, Work::GlsarState, state))) return rc;
    ExtraOut xo;
    xo.add(ro->se, a.se, sizeof(double) * G * kt);
    xo.add(ro->t_values, a.t_values, sizeof(double) * G * kt);
    xo.add(ro->p_values, a.p_values, sizeof(double) * G * kt);
    xo.add(ro->cov, a.cov, sizeof(double) * G * kt * kt);
    xo.add(ro->sigma2, a.sigma2, sizeof(double) * G);
    xo.add(ro->rho, a.rho, sizeof(double) * G);
    xo.add(ro->dw, a.dw, sizeof(double) * G);
    xo.add(ro->dw_ols, a.dw_ols, sizeof(double) * G);
    xo.add(ro->n_iter, a.n_iter, sizeof(int32_t) * G);
    xo.add(ro->n_obs, a.n_obs, sizeof(int64_t) * G);
    if ((rc = xo.place(ctx, fc, Work::GlsarOut))) return rc;
    ctx->last_kernel = sg.n_seg > 0 ? "k18_glsar_split" : "k18_glsar";
    if ((rc = k18_gram_launch(ctx, b->dtype, a))) return rc;
    if ((rc = k18_solve_launch(ctx, b->dtype, a))) return rc;
    if (need_rows) {
        if ((rc = k18_rows_launch(ctx, b->dtype, a))) return rc;
        if ((rc = k18_finish_launch(ctx, a))) return rc;
    }
    if ((rc = fit_predict(ctx, b, fc, &sg, a.x, a.k_user, kt, a.coefp))) return rc;
    return xo.home(ctx, b, o, fc);
}

void pols_absorb_params_default(pols_absorb_params *q) {
    if (!q) return;
    q->ids = nullptr;
    q->cov_type = POLS_COV_NONROBUST;
}

// K16 (k16_absorb.hip): K7c's order builder on the id column, the categories (run starts, their prefix, the index of every row), the
// means per category, the moments of the demeaned rows, the per-group solve, the residual pass per category and the per-group finish
// (only when a wanted output needs a residual), then the prediction pass.
int pols_least_squares_absorb(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_absorb_params *q, pols_out *o,
                              const pols_absorb_out *ro) {
    FitCall fc;
    int rc = fit_check(ctx, b, p, q, o, "absorb", K16_KMAX, &fc);
    if (rc) return rc;
    ro = or_none(ro);
    if ((rc = absorb_check(b, p, o, fc, "absorb", &q->ids, 1, q->cov_type, nullptr, ro->fe, nullptr))) return rc;
    if (b->n_groups == 0) return POLS_OK;
    const int k = b->n_features;
    const size_t G = fc.G, N = (size_t)b->n_rows;
    const bool cluster = q->cov_type == POLS_COV_CLUSTER;
    if ((rc = fit_stage(ctx, b, o, &fc))) return rc;
    AbsorbArgs a = {};
    fit_frame(a, b, fc);
    a.kt = k + 1; a.icpt = b->add_intercept ? 1 : 0; a.cluster = cluster ? 1 : 0;
    a.pred = fc.st.pred; a.resid = fc.st.resid;
    if ((rc = stage_ids(ctx, fc, Work::AbsorbIds, &q->ids, 1, N, &a.ids))) return rc;
    SegTables sg;
    if ((rc = ensure_segments(ctx, b, fc.max_rows, 0, &sg))) return rc;
    fit_segments(a, sg);
    const size_t items = sg.n_seg > 0 ? (size_t)sg.n_seg : G;
    if ((rc = k7c_order_launch(ctx, a.ids, fc.d_offs, b->n_groups, b->n_rows, &a.order))) return rc;
    if ((rc = categories(ctx, Work::AbsorbIndex, &a, 1, items, N))) return rc;
    POLS_HIP(hipStreamSynchronize(ctx->stream));                   // the number of categories sizes the table
    const size_t nc = (size_t)a.n_cats;
    Carve cats, moments;
    cats.add(a.cat_start, sizeof(int64_t) * (nc + 1)); cats.add(a.cat, sizeof(double) * nc * k16_cat_stride(k) + 8);
    cats.add(a.resid_part, sizeof(double) * nc * k16_resid_stride(k, cluster) + 8);
    moments.add(a.gram_part, sizeof(double) * items * k16_gram_stride(k)); moments.add(a.state, sizeof(double) * G * k16_state_stride(k));
    if ((rc = carve(ctx, Work::AbsorbCats, cats))) return rc;
    if ((rc = carve(ctx, Work::AbsorbMoments, moments))) return rc;
    ExtraOut xo;
    const bool need_rows = absorb_stats_out(xo, a, ro, G, fc.kt);
    xo.add(ro->fe, a.fe, fc.sz * N);
    xo.add(ro->n_obs, a.n_obs, sizeof(int64_t) * G); xo.add(ro->n_categories, a.n_categories, sizeof(int64_t) * G);
    if ((rc = xo.place(ctx, fc, Work::AbsorbOut))) return rc;
    ctx->last_kernel = a.order ? "k16_absorb_ordered" : "k16_absorb_sorted";
    if ((rc = k16_index_launch(ctx, a))) return rc;
    if ((rc = k16_means_launch(ctx, b->dtype, a))) return rc;
    if ((rc = k16_gram_launch(ctx, b->dtype, a))) return rc;
    if ((rc = k16_solve_launch(ctx, a))) return rc;
    if (need_rows) {
        if ((rc = k16_resid_launch(ctx, b->dtype, a))) return rc;
        if ((rc = k16_finish_launch(ctx, a))) return rc;
    }
    if ((rc = k16_predict_launch(ctx, b->dtype, a))) return rc;
    return xo.home(ctx, b, o, fc);
}

void pols_random_effects_params_default(pols_random_effects_params *q) {
    if (!q) return;
    q->ids = nullptr;
}

// K19 (k19_random_effects.hip): K16's launches as they are on an AbsorbArgs -- order, categories, index, means, moments, solve, the
// residual pass and the finish for sigma2_e --, then the table kernel (resident, global, or one of each over a group list when the
// frame has groups on both sides of the resident capacity), K16's residual pass again with b and the finish (only when se / t / p are
// wanted), then the prediction pass.  Two synchronisations: the order probe, the category counts.
int pols_random_effects(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_random_effects_params *q, pols_out *o,
                        const pols_random_effects_out *ro) {
    FitCall fc;
    int rc = fit_check(ctx, b, p, q, o, "random_effects", K19_KMAX, &fc);
    if (rc) return rc;
    ro = or_none(ro);
    if ((rc = absorb_check(b, p, o, fc, "random_effects", &q->ids, 1, POLS_COV_NONROBUST, nullptr, ro->effects, ro->theta))) return rc;
    if (b->weights) return fail(POLS_ERR_UNSUPPORTED, "random_effects: weights are not built");
    if (b->n_groups == 0) return POLS_OK;
    const int k = b->n_features, kc = fc.kt;
    const size_t G = fc.G, N = (size_t)b->n_rows;
    if ((rc = fit_stage(ctx, b, o, &fc))) return rc;
    AbsorbArgs a = {};                                             // the within fit: no coefficient, status or row output of its own
    fit_frame(a, b, fc);
    a.kt = k + 1; a.coef = nullptr; a.status = nullptr;
    if ((rc = stage_ids(ctx, fc, Work::RandomEffectsIds, &q->ids, 1, N, &a.ids))) return rc;
    SegTables sg;
    if ((rc = ensure_segments(ctx, b, fc.max_rows, 0, &sg))) return rc;
    fit_segments(a, sg);
    const size_t items = sg.n_seg > 0 ? (size_t)sg.n_seg : G;
    RandomEffectsArgs r = {};
    fit_frame(r, b, fc);
    fit_segments(r, sg);
    int32_t *list = nullptr;
    Carve moments;
    moments.add(a.gram_part, sizeof(double) * items * k16_gram_stride(k)); moments.add(a.state, sizeof(double) * G * k16_state_stride(k));
    moments.add(a.sigma2, sizeof(double) * G); moments.add(r.state, sizeof(double) * G * k19_state_stride(kc));
    moments.add(r.rstate, sizeof(double) * G * k16_state_stride(k)); moments.add(r.table_rows, sizeof(int64_t) * G);
    moments.add(list, sizeof(int32_t) * G);
    if ((rc = carve(ctx, Work::RandomEffectsMoments, moments))) return rc;
    if ((rc = k7c_order_launch(ctx, a.ids, fc.d_offs, b->n_groups, b->n_rows, &a.order))) return rc;
    if ((rc = categories(ctx, Work::RandomEffectsIndex, &a, 1, items, N))) return rc;
    r.item_first = a.item_first; r.catidx = a.catidx;
    if ((rc = k19_rows_launch(ctx, r))) return rc;
    std::vector<int64_t> table_rows(G);
    POLS_HIP(hipMemcpyAsync(table_rows.data(), r.table_rows, sizeof(int64_t) * G, hipMemcpyDeviceToHost, ctx->stream));
    POLS_HIP(hipStreamSynchronize(ctx->stream));                   // the number of categories sizes the table, their counts per group pick the route
    const size_t nc = (size_t)a.n_cats;
    // which groups the resident table kernel takes: by the rows of the table they span
    const K19Split sp = k19_split_groups(table_rows.data(), G, ctx->opt.random_effects_route == 1 ? -1 : k19_resident_rows(k, kc, (long long)FIT_LDS_BUDGET));
    if (sp.mixed() && (rc = upload_small(ctx, list, sp.list.data(), sizeof(int32_t) * G))) return rc;
    double *rss_rows = nullptr;
    Carve cats;
    cats.add(a.cat_start, sizeof(int64_t) * (nc + 1)); cats.add(a.cat, sizeof(double) * nc * k16_cat_stride(k) + 8);
    cats.add(a.resid_part, sizeof(double) * nc + 8); cats.add(rss_rows, sizeof(double) * nc + 8);
    cats.add(r.theta_c, sizeof(double) * nc + 8); cats.add(r.u_c, sizeof(double) * nc + 8); cats.add(r.q_c, sizeof(double) * nc + 8);
    if ((rc = carve(ctx, Work::RandomEffectsCats, cats))) return rc;
    ExtraOut xo;
    xo.add(ro->se, r.se, sizeof(double) * G * kc); xo.add(ro->t_values, r.t_values, sizeof(double) * G * kc);
    xo.add(ro->p_values, r.p_values, sizeof(double) * G * kc);
    xo.add(ro->coef_between, r.coef_between, sizeof(double) * G * kc); xo.add(ro->coef_within, r.coef_within, sizeof(double) * G * k);
    xo.add(ro->sigma2_e, r.sigma2_e_out, sizeof(double) * G); xo.add(ro->sigma2_u, r.sigma2_u, sizeof(double) * G);
    xo.add(ro->rho, r.rho, sizeof(double) * G); xo.add(ro->hausman, r.hausman, sizeof(double) * G);
    xo.add(ro->hausman_p, r.hausman_p, sizeof(double) * G);
    xo.add(ro->effects, r.effects, fc.sz * N); xo.add(ro->theta, r.theta, fc.sz * N);
    xo.add(ro->n_obs, a.n_obs, sizeof(int64_t) * G); xo.add(ro->n_categories, a.n_categories, sizeof(int64_t) * G);
    if ((rc = xo.place(ctx, fc, Work::RandomEffectsOut))) return rc;
    const bool need_rows = ro->se || ro->t_values || ro->p_values;
    ctx->last_kernel = sp.mixed() ? "k19_random_effects_mixed" : (sp.n_res > 0 ? "k19_random_effects_resident" : "k19_random_effects_global");
    // 1. within: K16 unchanged; its residual pass and finish give sigma2_e
    if ((rc = k16_index_launch(ctx, a))) return rc;
    if ((rc = k16_means_launch(ctx, b->dtype, a))) return rc;
    if ((rc = k16_gram_launch(ctx, b->dtype, a))) return rc;
    if ((rc = k16_solve_launch(ctx, a))) return rc;
    if ((rc = k16_resid_launch(ctx, b->dtype, a))) return rc;
    if ((rc = k16_finish_launch(ctx, a))) return rc;
    // 2. - 8. the table kernel
    r.cat = a.cat; r.gram_part = a.gram_part; r.wstate = a.state; r.sigma2_e = a.sigma2;
    r.res_rows = (int32_t)sp.max_res;
    if (sp.mixed()) {
        RandomEffectsArgs part = r;
        part.list = list;
        if ((rc = k19_table_launch(ctx, part, true, sp.n_res))) return rc;
        part.list = list + sp.n_res;
        if ((rc = k19_table_launch(ctx, part, false, sp.n_glb))) return rc;
    } else if ((rc = k19_table_launch(ctx, r, sp.n_res > 0, (int64_t)G))) return rc;
    if (need_rows) {                                               // the row term of RSS: K16's residual pass on the state row that holds b
        AbsorbArgs rows = a;
        rows.state = r.rstate; rows.resid_part = rss_rows;
        if ((rc = k16_resid_launch(ctx, b->dtype, rows))) return rc;
        r.resid_part = rss_rows;
        if ((rc = k19_finish_launch(ctx, r))) return rc;
    }
    r.pred = fc.st.pred; r.resid = fc.st.resid;
    if ((rc = k19_predict_launch(ctx, b->dtype, r))) return rc;
    return xo.home(ctx, b, o, fc);
}

void pols_absorb2_params_default(pols_absorb2_params *q) {
    if (!q) return;
    q->ids = nullptr;
    q->ids2 = nullptr;
    q->cov_type = POLS_COV_NONROBUST;
    q->max_iter = 10000;
    q->tol = 1e-10;
}

// K17 (k17_absorb2.hip): K7c's order builder and K16's category launches on each id column, the stage launch (the rows in id-1 order,
// perm2), the demean launch -- resident, global, or one of each over a group list when the frame has groups on both sides of the
// resident capacity --, the moments of the demeaned columns, the per-group solve, the residual pass per id-1 category and the per-group
// finish (only when a wanted output needs a residual), then the prediction pass.  Three synchronisations: two order builds, one count copy.
int pols_least_squares_absorb2(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_absorb2_params *q, pols_out *o,
                               const pols_absorb2_out *ro) {
    FitCall fc;
    int rc = fit_check(ctx, b, p, q, o, "absorb2", K17_KMAX, &fc);
    if (rc) return rc;
    ro = or_none(ro);
    const int64_t *ids[2] = {q->ids, q->ids2}, *d_ids[2] = {nullptr, nullptr};
    if ((rc = absorb_check(b, p, o, fc, "absorb2", ids, 2, q->cov_type, q, ro->fe1, ro->fe2))) return rc;
    if (b->n_groups == 0) return POLS_OK;
    const int k = b->n_features;
    const size_t G = fc.G, N = (size_t)b->n_rows;
    const bool cluster = q->cov_type == POLS_COV_CLUSTER;
    if ((rc = fit_stage(ctx, b, o, &fc))) return rc;
    Absorb2Args a = {};
    fit_frame(a, b, fc);
    a.kt = k + 1; a.icpt = b->add_intercept ? 1 : 0; a.cluster = cluster ? 1 : 0;
    a.has_w = (fc.st.w || (fc.pol != POLS_NULL_IGNORE && fc.pol != POLS_NULL_ZERO)) ? 1 : 0;
    a.max_iter = q->max_iter; a.tol = q->tol;
    a.pred = fc.st.pred; a.resid = fc.st.resid;
    if ((rc = stage_ids(ctx, fc, Work::Absorb2Ids, ids, 2, N, d_ids))) return rc;
    SegTables sg;
    if ((rc = ensure_segments(ctx, b, fc.max_rows, 0, &sg))) return rc;
    fit_segments(a, sg);
    const size_t items = sg.n_seg > 0 ? (size_t)sg.n_seg : G;
    // which groups the resident store takes: by their rows alone (k17_resident_bytes lays the start tables out for C = n)
    const K17Split sp = k17_split_groups(b->group_offsets, G, ctx->opt.absorb2_route == 1 ? -1 : k17_resident_rows(a.has_w != 0));
    const int32_t *d_list = nullptr;
    if ((rc = absorb2_orders(ctx, b, fc, d_ids, sp, a, &d_list))) return rc;
    // the categories of each id column: K16's launches on an AbsorbArgs that names the column, its order and its tables
    AbsorbArgs way[2] = {};
    for (int w = 0; w < 2; ++w) {
        way[w].offs = fc.d_offs; way[w].n_groups = b->n_groups; way[w].n_rows = b->n_rows;
        fit_segments(way[w], sg);
        way[w].ids = d_ids[w]; way[w].order = w ? a.order2 : a.order1;
    }
    if ((rc = categories(ctx, Work::Absorb2Index, way, 2, items, N))) return rc;
    POLS_HIP(hipStreamSynchronize(ctx->stream));                   // the numbers of categories size the tables
    if ((rc = absorb2_tables(ctx, a, way, items, G, N, k, cluster))) return rc;
    for (int w = 0; w < 2; ++w)
        if ((rc = k16_index_launch(ctx, way[w]))) return rc;
    a.first1 = way[0].item_first; a.first2 = way[1].item_first;
    a.catidx1 = way[0].catidx; a.catidx2 = way[1].catidx;
    a.start1 = way[0].cat_start; a.start2 = way[1].cat_start;
    a.n_cats1 = way[0].n_cats; a.n_cats2 = way[1].n_cats;
    ExtraOut xo;
    const bool need_rows = absorb_stats_out(xo, a, ro, G, fc.kt);
    xo.add(ro->fe1, a.fe1, fc.sz * N); xo.add(ro->fe2, a.fe2, fc.sz * N);
    xo.add(ro->n_obs, a.n_obs, sizeof(int64_t) * G); xo.add(ro->n_categories, a.n_categories, sizeof(int64_t) * G);
    xo.add(ro->n_categories2, a.n_categories2, sizeof(int64_t) * G); xo.add(ro->n_components, a.n_components, sizeof(int64_t) * G);
    xo.add(ro->n_iter, a.n_iter, sizeof(int32_t) * G);
    if ((rc = xo.place(ctx, fc, Work::Absorb2Out))) return rc;
    ctx->last_kernel = sp.mixed() ? "k17_absorb2_mixed" : (sp.n_res > 0 ? "k17_absorb2_resident" : "k17_absorb2_global");
    if ((rc = absorb2_launches(ctx, b->dtype, a, sp, d_list, need_rows))) return rc;
    return xo.home(ctx, b, o, fc);
}

void pols_enet_cv_params_default(pols_enet_cv_params *q) {
    if (!q) return;
    q->alphas = nullptr;
    q->n_alphas = 100;
    q->eps = 1e-3;
    q->l1_ratio = 0.5;
    q->n_folds = 5;
    q->max_iter = 1000;
    q->tol = 1e-5;
    q->positive = 0;
}

// K12 (k12_enet_cv.hip): fold Gram matrices in one pass over the frame (behind a count pass when the null policy can remove rows),
// the (n_folds + 1) x n_alphas coordinate-descent fits on chip, pick, then K10's prediction pass with the winner's coefficients.
int pols_elastic_net_cv(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_enet_cv_params *q, pols_out *o,
                        const pols_enet_cv_out *ro) {
    FitCall fc;
    int rc = fit_check(ctx, b, p, q, o, "elastic_net_cv", K12_KMAX, &fc);
    if (rc) return rc;
    const bool automatic = q->alphas == nullptr;
    if (!(q->l1_ratio >= 0.0 && q->l1_ratio <= 1.0)) return fail(POLS_ERR_INVALID, "elastic_net_cv: l1_ratio %g outside [0, 1]", q->l1_ratio);
    if (q->n_alphas < 1) return fail(POLS_ERR_INVALID, "elastic_net_cv: the grid of candidates is empty");
    if (q->n_alphas > K12_MAX_ALPHAS) return fail(POLS_ERR_UNSUPPORTED, "elastic_net_cv: %d candidates > %d", q->n_alphas, K12_MAX_ALPHAS);
    if (automatic) {
        if (q->n_alphas < 2) return fail(POLS_ERR_INVALID, "elastic_net_cv: an automatic grid needs at least 2 candidates");
        if (!(q->eps > 0.0 && q->eps < 1.0)) return fail(POLS_ERR_INVALID, "elastic_net_cv: eps %g outside (0, 1)", q->eps);
        if (q->l1_ratio == 0.0) return fail(POLS_ERR_INVALID, "elastic_net_cv: an automatic grid needs l1_ratio > 0");
    } else {
        for (int j = 0; j < q->n_alphas; ++j)
            if (!(q->alphas[j] >= 0.0) || !std::isfinite(q->alphas[j])) return fail(POLS_ERR_INVALID, "elastic_net_cv: candidate %d is negative or not finite", j);
    }
    if (q->n_folds < 2 || q->n_folds > K12_MAX_FOLDS) return fail(POLS_ERR_INVALID, "elastic_net_cv: %d folds outside 2..%d", q->n_folds, K12_MAX_FOLDS);
    if (q->max_iter < 1) return fail(POLS_ERR_INVALID, "elastic_net_cv: max_iter %d < 1", q->max_iter);
    if (!(q->tol > 0.0) || !std::isfinite(q->tol)) return fail(POLS_ERR_INVALID, "elastic_net_cv: tol %g is not positive and finite", q->tol);
    if (b->n_groups == 0) return POLS_OK;
    ro = or_none(ro);
    if ((rc = fit_stage(ctx, b, o, &fc))) return rc;
    const int kt = fc.kt, na = q->n_alphas, nf = q->n_folds, pol = fc.pol;
    const size_t G = fc.G;
    SegTables sg;
    if ((rc = ensure_segments(ctx, b, fc.max_rows, 0, &sg))) return rc;
    const bool split = sg.n_seg > 0;
    const size_t items = split ? (size_t)sg.n_seg : G;
    const size_t per = (size_t)nf * k10_gram_stride(kt);
    EnetCvArgs a = {};
    fit_frame(a, b, fc);
    fit_segments(a, sg);
    a.n_folds = nf; a.n_alphas = na; a.automatic = automatic ? 1 : 0;
    a.counted = (pol == POLS_NULL_DROP || pol == POLS_NULL_DROP_ZERO || pol == POLS_NULL_DROP_WINDOW || pol == POLS_NULL_DROP_Y_ZERO_X) ? 1 : 0;
    a.max_iter = q->max_iter; a.positive = q->positive ? 1 : 0;
    a.l1_ratio = q->l1_ratio; a.tol = q->tol; a.eps = q->eps;
    // the candidates and the order they are visited in share one region: n_alphas doubles, then n_alphas int32
    std::vector<char> up(sizeof(double) * (size_t)na + sizeof(int32_t) * (size_t)na);
    char *packed = nullptr;
    Carve gram, work;
    gram.add(a.item_count, sizeof(int64_t) * items); gram.add(a.fold_part, sizeof(double) * items * per);
    gram.add(a.fold_gram, split ? sizeof(double) * G * per : 0, &a.fold_part);   // (nothing is split: the parts are the matrices)
    work.add(packed, up.size()); work.add(a.score_part, sizeof(double) * G * nf * (size_t)na);
    work.add(a.iters, sizeof(int32_t) * G * (nf + 1) * (size_t)na); work.add(a.path64, sizeof(double) * G * (size_t)na * kt);
    work.add(a.grid, sizeof(double) * G * (size_t)na); work.add(a.coef64, sizeof(double) * G * kt);
    if ((rc = carve(ctx, Work::EnetCvGram, gram))) return rc;
    if ((rc = carve(ctx, Work::EnetCvWork, work))) return rc;
    double *ua = reinterpret_cast<double *>(up.data());             // descending alpha, equal values in index order
    int32_t *uo = reinterpret_cast<int32_t *>(up.data() + sizeof(double) * (size_t)na);
    for (int j = 0; j < na; ++j) { ua[j] = automatic ? 0.0 : q->alphas[j]; uo[j] = j; }
    if (!automatic) std::stable_sort(uo, uo + na, [&](int32_t x, int32_t y) { return ua[x] > ua[y]; });
    if ((rc = upload_small(ctx, packed, up.data(), up.size()))) return rc;
    a.alphas = reinterpret_cast<const double *>(packed);
    a.order = reinterpret_cast<const int32_t *>(packed + sizeof(double) * (size_t)na);
    ExtraOut xo;
    xo.add(ro->alpha, a.alpha, sizeof(double) * G);
    xo.add(ro->score, a.score, sizeof(double) * G);
    xo.add(ro->alpha_index, a.alpha_index, sizeof(int32_t) * G);
    xo.add(ro->cv_scores, a.cv_scores, sizeof(double) * G * (size_t)na);
    xo.add(ro->alphas_used, a.alphas_used, sizeof(double) * G * (size_t)na);
    xo.add(ro->coef_path, a.coef_path, fc.sz * G * (size_t)na * kt);
    xo.add(ro->n_iter, a.n_iter, sizeof(int32_t) * G * (size_t)na);
    if ((rc = xo.place(ctx, fc, Work::EnetCvOut))) return rc;
    ctx->last_kernel = split ? "k12_enet_cv_split" : "k12_enet_cv";
    if ((rc = k12_count_launch(ctx, b->dtype, a))) return rc;
    if ((rc = k12_fold_gram_launch(ctx, b->dtype, a))) return rc;
    if ((rc = k12_reduce_launch(ctx, a))) return rc;
    if ((rc = k12_path_launch(ctx, a))) return rc;
    if ((rc = k12_pick_launch(ctx, a))) return rc;
    if ((rc = fit_predict(ctx, b, fc, &sg, a.x, a.k_user, kt, a.coef64))) return rc;
    return xo.home(ctx, b, o, fc);
}

}  // extern "C"
