// api_stats.hip -- mode = "statistics": pols_least_squares_statistics, its robust and cluster twins and pols_least_squares_influence.
// One call description (StatsCall), two levels -- statistics_filtered applies a null policy and hands the rows it leaves to statistics_fit,
// which never sees a null -- and one function per stage inside the fit level.  DESIGN.md "Statistics mode" has the table of stages, the work
// areas each owns and the ordering rules.
#include <algorithm>
#include <cstring>
#include <utility>

#include "common.hpp"
#include "api_internal.hpp"
#include "k5_enet.hpp"
#include "k7_stats.hpp"
#include "k7r_robust.hpp"
#include "k7c_cluster.hpp"
#include "k7i_influence.hpp"
#include "k8_wide.hpp"

namespace pols {
namespace {     // (the types of this file: their inline members stay out of the library's dynamic symbols)

// ------------------------------------------------------------------ the call
// Which of the four entries a call came through, and the one parameter block that entry validated: pols_cov_params (Robust: HC0 .. HAC, at
// most K7_KMAX columns), pols_cluster_params (Cluster), pols_influence_params (Influence, with the per-row outputs in `rows`); nothing for Plain.
enum class StatsKind { Plain, Robust, Cluster, Influence };
struct StatsCall {
    StatsKind kind = StatsKind::Plain;
    const void *params = nullptr;
    const pols_influence_out *rows = nullptr;
    const pols_cov_params *cov() const { return kind == StatsKind::Robust ? static_cast<const pols_cov_params *>(params) : nullptr; }
    const pols_cluster_params *cl() const { return kind == StatsKind::Cluster ? static_cast<const pols_cluster_params *>(params) : nullptr; }
    const pols_influence_params *infl() const { return kind == StatsKind::Influence ? static_cast<const pols_influence_params *>(params) : nullptr; }
};
static int cluster_ways(const pols_cluster_params *cl) { return cl->cov_type == POLS_COV_CLUSTER2 ? 2 : 1; }

// ------------------------------------------------------------------ the six statistic arrays
// r2 / mae / mse (one double per group) and std_err / t_values / p_values (kt per group), in pols_stats_out's order: where the caller wants
// them, where the kernels write them, and the copy home.  As constructed the kernels write the caller's device arrays; stage() adds the
// six to the buffer the caller is carving (Work::CompactOut, Work::HostStaged, Work::Tables).  Every one keeps its room whether or not it
// is wanted: the buffer of a frame does not depend on what was asked for.  (The carve holds the addresses of dev[]: stage the object
// where it stays.)
struct SixOut {
    double *user[6] = {}, *dev[6] = {};
    size_t G = 0;
    int kt = 0;
    size_t bytes(int i) const { return sizeof(double) * G * (size_t)(i < 3 ? 1 : kt); }
    SixOut() = default;
    SixOut(const pols_stats_out *s, size_t G_, int kt_) : G(G_), kt(kt_) {
        double *const u[6] = {s->r2, s->mae, s->mse, s->std_err, s->t_values, s->p_values};
        for (int i = 0; i < 6; ++i) user[i] = dev[i] = u[i];
    }
    // staged (host batches): the wanted ones are written into the buffer; else only their room is kept
    void stage(Carve &cv, bool staged) {
        for (int i = 0; i < 6; ++i) {
            if (staged) cv.keep(dev[i], bytes(i), user[i] != nullptr);
            else cv.gap(bytes(i));
        }
    }
    pols_stats_out on_device() const { pols_stats_out d; d.r2 = dev[0]; d.mae = dev[1]; d.mse = dev[2]; d.std_err = dev[3]; d.t_values = dev[4]; d.p_values = dev[5]; return d; }
    int copy_home(pols_ctx *ctx) const {           // (staged arrays only: asynchronous, the caller synchronises)
        for (int i = 0; i < 6; ++i)
            if (user[i]) POLS_HIP(hipMemcpyAsync(user[i], dev[i], bytes(i), hipMemcpyDeviceToHost, ctx->stream));
        return POLS_OK;
    }
};

// ------------------------------------------------------------------ the coefficients nobody asked for
// The statistics kernels read the coefficients whether or not the caller wants them.  A device batch gets `spare` device bytes for them; a
// host batch stages every non-NULL output, so the address of a one-byte object asks stage_inputs for staged coefficients -- and home() takes
// it back before unstage_outputs, which would otherwise copy the coefficients from the device into that one byte.
struct CoefAsk {
    pols_out oo;
    bool asked = false;
    char sentinel = 0;
    CoefAsk() { std::memset(&oo, 0, sizeof(oo)); }
    CoefAsk(const CoefAsk &) = delete;
    CoefAsk &operator=(const CoefAsk &) = delete;
    void ask(const pols_out *o, bool host, void *spare) {
        oo = *o;
        asked = !o->coef;
        if (asked) oo.coef = host ? static_cast<void *>(&sentinel) : spare;
    }
    int home(pols_ctx *ctx, const pols_batch *b, int kt, const Staged &st) {
        if (asked) oo.coef = nullptr;
        return unstage_outputs(ctx, b, b->n_groups, kt, &oo, st);
    }
};

// What the fit level leaves behind: what a row pass over the fitted rows needs (staged columns, device offsets, segment tables), the group
// stage's tables of an influence call, and what fit_home copies back for a host batch.
struct Fit {
    Staged st;
    const int64_t *d_offs = nullptr;
    SegTables sg;
    double *infl_prep = nullptr, *infl_grp = nullptr;   // Work::InflPrep; Work::InflGroup behind the RSS
    SixOut six;
    CoefAsk coef;
};

}  // namespace

// ------------------------------------------------------------------ cluster ids, influence rows
// The ids of a batch's rows on the device: the caller's own for a device batch, staged into Work::ClusterIds for a host batch.
static int cluster_device_ids(pols_ctx *ctx, const pols_batch *b, const pols_cluster_params *cl, int ways, const int64_t **dev) {
    if (b->mem == POLS_MEM_DEVICE) {
        for (int w = 0; w < ways; ++w) dev[w] = cl->ids[w];
        return POLS_OK;
    }
    const size_t colb = round256(sizeof(int64_t) * (size_t)std::max<int64_t>(b->n_rows, 1));
    int64_t *ids = nullptr;
    Carve cv;
    cv.add(ids, colb * (size_t)ways);
    int rc = carve(ctx, Work::ClusterIds, cv);
    if (rc) return rc;
    for (int w = 0; w < ways; ++w) {
        int64_t *dst = column(ids, colb, (size_t)w);
        if (b->n_rows) POLS_HIP(hipMemcpyAsync(dst, cl->ids[w], sizeof(int64_t) * (size_t)b->n_rows, hipMemcpyHostToDevice, ctx->stream));
        dev[w] = dst;
    }
    return POLS_OK;
}

// The row pass of K7i (k7i_influence.hip) over the rows of `b` as staged in `st`, then the per-group outputs; valid == nullptr: every row was
// fitted.  Called by the level that owns the ORIGINAL rows: statistics_filtered under a null policy, statistics_run otherwise.
static int influence_rows(pols_ctx *ctx, const pols_batch *b, const Staged &st, const int64_t *d_offs, const SegTables &sg, const uint8_t *valid,
                          int zero_fill, const pols_influence_out *io, const Fit &f) {
    const bool host = b->mem == POLS_MEM_HOST;
    const size_t G = (size_t)b->n_groups, N = (size_t)b->n_rows, sz = dtype_size(b->dtype), colb = round256(sz * std::max<size_t>(N, 1));
    void *const user[K7I_NOUT] = {io->leverage, io->student_internal, io->student_external, io->cooks_d, io->dffits, io->se_mean,
                                  io->se_obs, io->mean_lo, io->mean_hi, io->obs_lo, io->obs_hi};
    int rc, n_out = 0;
    for (int i = 0; i < K7I_NOUT; ++i) n_out += user[i] ? 1 : 0;
    InflArgs a;
    std::memset(&a, 0, sizeof(a));
    a.y = st.y; a.w = st.w;
    for (int j = 0; j < b->n_features; ++j) a.x[j] = st.x[(size_t)j];
    a.offs = d_offs; a.n_groups = b->n_groups; a.n_rows = b->n_rows;
    if (sg.n_seg > 0) { a.seg_offs = sg.offs; a.seg_map = sg.map; a.n_seg = sg.n_seg; }
    a.valid = valid; a.zero_fill = zero_fill;
    a.k_user = b->n_features; a.kt = b->n_features + (b->add_intercept ? 1 : 0);
    a.prep = f.infl_prep; a.grp = f.infl_grp;
    void *rows = nullptr;                             // one column per wanted output of a host batch: what is not wanted takes no room
    Carve cv;
    cv.add(rows, host ? colb * (size_t)n_out : 0);
    if (host && n_out && (rc = carve(ctx, Work::InflRows, cv))) return rc;
    for (int i = 0, at = 0; i < K7I_NOUT; ++i) {
        if (!user[i]) continue;
        if (!host && !aligned16(user[i])) return fail(POLS_ERR_INVALID, "device columns must be 16-byte aligned");
        a.out[i] = host ? column(rows, colb, (size_t)at++) : user[i];
    }
    if ((rc = k7i_rows_launch(ctx, b->dtype, a))) return rc;
    if (host && N)
        for (int i = 0; i < K7I_NOUT; ++i)
            if (user[i]) POLS_HIP(hipMemcpyAsync(user[i], a.out[i], sz * N, hipMemcpyDeviceToHost, ctx->stream));
    double *const gu[3] = {io->sigma2, io->df, io->t_crit};
    for (int i = 0; i < 3; ++i)
        if (gu[i]) POLS_HIP(hipMemcpyAsync(gu[i], f.infl_grp + (size_t)i * G, sizeof(double) * G, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    return POLS_OK;
}

// ------------------------------------------------------------------ the fit level: one function per stage
// 32 .. 1 024 columns: the K8 kernels solve (same dispatcher), then the wide statistics kernel works from their Gram matrix.
// Work::HostStaged: the six arrays of a host batch.
static int stats_wide(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_out *o, const pols_stats_out *s, int kt, Fit *f) {
    const bool host = b->mem == POLS_MEM_HOST;
    const size_t G = (size_t)b->n_groups;
    int rc;
    SolvePlan plan;
    if ((rc = resolve_solve_plan(p, b->dtype, kt, 1, &plan))) return rc;
    f->six = SixOut(s, G, kt);
    if (host) {
        Carve cv;
        f->six.stage(cv, true);
        if ((rc = carve(ctx, Work::HostStaged, cv))) return rc;
    }
    f->coef.ask(o, host, nullptr);                  // (a device batch without coefficients: wide_static keeps its own)
    WideInfo wi;
    if ((rc = wide_static(ctx, b, p, &f->coef.oo, kt, plan, nullptr, 1, nullptr, &wi))) return rc;
    f->st = std::move(wi.st);
    WideStatsOut so;
    so.r2 = f->six.dev[0]; so.mae = f->six.dev[1]; so.mse = f->six.dev[2]; so.se = f->six.dev[3]; so.tv = f->six.dev[4]; so.pv = f->six.dev[5];
    so.lambda = p->alpha;
    so.factored = !plan.enet() && kt + 1 > 128;     // wide_chol ran on the Gram matrix in place (k8_wide.hip)
    return wide_stats_launch(ctx, b->dtype, wi.a, so);
}

// The Gram matrices Z'Z of every group (Z = [sqrt(w) X | sqrt(w) 1 | sqrt(w) y]): the solve's own when its streamed route ran over the whole
// frame, else one streamed pass into Work::Gram.  Long groups (the size-class + streamed route of ls_core keeps no per-group Gram matrices)
// take the segment split of the streamed path here too -- an unsplit launch is one workgroup per group, i.e. ONE CU for a multi-million-row
// group: per-segment partials in the segment cache's extra area, reduced per group (through 16 slices in Work::Fixup, idle here, when one
// group has hundreds of segments).  K7's segment sums reuse that extra area AFTER the reduce, on the same stream.
static int stats_gram(pols_ctx *ctx, const pols_batch *b, int kt, const Fit &f, double *solve_gram, double **gram) {
    if ((*gram = solve_gram)) return POLS_OK;
    const size_t G = (size_t)b->n_groups, nz = (size_t)kt + 1;
    int rc;
    void *gs = nullptr;
    if ((rc = ensure_scratch(ctx, Work::Gram, round256(sizeof(double) * nz * nz * G), &gs))) return rc;
    *gram = static_cast<double *>(gs);
    GramArgs ga;
    std::memset(&ga, 0, sizeof(ga));
    ga.y = f.st.y; ga.w = f.st.w;
    for (int j = 0; j < b->n_features; ++j) ga.x[j] = f.st.x[j];
    ga.offs = f.d_offs; ga.n_groups = b->n_groups; ga.n_rows = b->n_rows;
    ga.gram = *gram;
    ga.k_user = b->n_features; ga.kt = kt;
    SegTables sg;
    if ((rc = ensure_segments(ctx, b, ctx->offs_max_rows, sizeof(double) * (nz * nz + 1), &sg))) return rc;
    if (sg.n_seg == 0) return gram_stream_launch(ctx, b->dtype, ga);
    const int n_slices = (sg.max_seg >= 256 && G <= 256) ? 16 : 1;
    void *sl = nullptr;
    if (n_slices > 1 && (rc = ensure_scratch(ctx, Work::Fixup, round256(sizeof(double) * nz * nz * (size_t)n_slices * G), &sl))) return rc;
    ga.offs = sg.offs; ga.n_groups = sg.n_seg; ga.gram = reinterpret_cast<double *>(sg.extra);
    if ((rc = gram_stream_launch(ctx, b->dtype, ga))) return rc;
    GramReduceArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    ra.part = ga.gram; ra.first = sg.first; ra.gram = *gram; ra.n_groups = b->n_groups; ra.nz2 = (int32_t)(nz * nz);
    ra.max_segments = (int32_t)std::min<int64_t>(1 << 30, sg.max_seg);
    if (n_slices > 1) { ra.slices = static_cast<double *>(sl); ra.n_slices = n_slices; }
    return gram_reduce_launch(ctx, ra);
}

// The arguments of K7 (and, copied, of the kernels that follow it) from what the fit has so far: staged columns, offsets, the six arrays.
// Long groups (ONE model summary over a whole frame): the row passes run per segment -- the frame's cached tables (f->sg, keyed by the
// offsets ls_core just uploaded: no O(groups) host loop per call), five partial sums per segment in their extra area, the per-group
// preparation in Work::RowCompact (the rolling entry's, never live here).
static int stats_args(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, int kt, double *gram, StatsArgs *sa, Fit *f) {
    std::memset(sa, 0, sizeof(*sa));
    sa->y = f->st.y; sa->w = f->st.w;
    for (int j = 0; j < b->n_features; ++j) sa->x[j] = f->st.x[j];
    sa->offs = f->d_offs; sa->n_groups = b->n_groups; sa->gram = gram;
    sa->coef = f->st.coef; sa->lambda = p->alpha; sa->status = f->st.status;
    sa->k_user = b->n_features; sa->kt = kt;
    double *const *dev = f->six.dev;
    sa->r2 = dev[0]; sa->mae = dev[1]; sa->mse = dev[2]; sa->se = dev[3]; sa->tv = dev[4]; sa->pv = dev[5];
    int rc;
    if ((rc = ensure_segments(ctx, b, ctx->offs_max_rows, sizeof(double) * 5, &f->sg))) return rc;
    if (f->sg.n_seg == 0) return POLS_OK;
    void *pp = nullptr;
    if ((rc = ensure_scratch(ctx, Work::RowCompact, round256(sizeof(double) * (size_t)b->n_groups * (3 * (size_t)kt + 1)), &pp))) return rc;
    sa->seg_offs = f->sg.offs; sa->seg_map = f->sg.map; sa->seg_first = f->sg.first; sa->n_seg = f->sg.n_seg;
    sa->seg_part = reinterpret_cast<double *>(f->sg.extra);
    sa->prep = static_cast<double *>(pp);
    return POLS_OK;
}

static int run_plain(pols_ctx *ctx, const pols_batch *b, const StatsArgs &sa) { return k7_stats_launch(ctx, b->dtype, sa); }

// K7 keeps r2 / mae / mse / status, the follow-up kernel (K7r, K7c) writes the standard errors, t- and p-values: `next` takes the arguments
// WITH se / tv / pv, K7 runs without them, then `launch`.  Both kernels have their own buffers (`prep`: A^-1 / b / trace / ok per group;
// `part`: part_doubles doubles of partial sums per segment or group): sa's segment tables are the frame's cached ones, the partial sums live apart.
template <typename Next>
static int k7_then(pols_ctx *ctx, const pols_batch *b, StatsArgs sa, Next &next, Work prep, Work part, size_t part_doubles,
                   int (*launch)(pols_ctx *, int, const Next &)) {
    int rc;
    next.s = sa;
    sa.se = sa.tv = sa.pv = nullptr;
    void *pr = nullptr, *pt = nullptr;
    if ((rc = ensure_scratch(ctx, prep, round256(sizeof(double) * (size_t)b->n_groups * k7r_prep_stride(sa.kt)), &pr))) return rc;
    if ((rc = ensure_scratch(ctx, part, round256(sizeof(double) * part_doubles), &pt))) return rc;
    next.prep = static_cast<double *>(pr);
    next.part = static_cast<double *>(pt);
    if ((rc = k7_stats_launch(ctx, b->dtype, sa))) return rc;
    return launch(ctx, b->dtype, next);
}
static size_t seg_items(const StatsArgs &sa) { return sa.seg_offs ? (size_t)sa.n_seg : (size_t)sa.n_groups; }

// HC0 .. HAC (K7r, k7r_robust.hip): Work::RobustPrep, Work::RobustMeat
static int run_robust(pols_ctx *ctx, const pols_batch *b, const pols_cov_params *cov, const StatsArgs &sa) {
    RobustArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    ra.cov_type = cov->cov_type;
    ra.maxlags = cov->cov_type == POLS_COV_HAC ? cov->maxlags : 0;
    return k7_then(ctx, b, sa, ra, Work::RobustPrep, Work::RobustMeat, seg_items(sa) * k7r_part_stride(sa.kt), k7r_robust_launch);
}

// One- / two-way cluster-robust (K7c, k7c_cluster.hip), which also counts the clusters: Work::ClusterPrep, Work::ClusterPart, and for a host
// batch Work::ClusterIds and Work::ClusterCounts
static int run_cluster(pols_ctx *ctx, const pols_batch *b, const pols_cluster_params *cl, const StatsArgs &sa) {
    const bool host = b->mem == POLS_MEM_HOST;
    const size_t G = (size_t)b->n_groups;
    int rc;
    ClusterArgs ca;
    std::memset(&ca, 0, sizeof(ca));
    ca.n_rows = b->n_rows;
    ca.ways = cluster_ways(cl);
    ca.use_correction = cl->use_correction ? 1 : 0;
    if ((rc = cluster_device_ids(ctx, b, cl, ca.ways, ca.ids))) return rc;
    void *nc = nullptr;
    if (cl->n_clusters && host && (rc = ensure_scratch(ctx, Work::ClusterCounts, round256(sizeof(int64_t) * G * (size_t)ca.ways), &nc))) return rc;
    ca.n_clusters = host ? static_cast<int64_t *>(nc) : cl->n_clusters;
    if ((rc = k7_then(ctx, b, sa, ca, Work::ClusterPrep, Work::ClusterPart, seg_items(sa) * k7c_part_stride(sa.kt) + 3 * G * ((size_t)sa.kt + 1),
                      k7c_cluster_launch)))
        return rc;
    if (host && cl->n_clusters)
        POLS_HIP(hipMemcpyAsync(cl->n_clusters, ca.n_clusters, sizeof(int64_t) * G * (size_t)ca.ways, hipMemcpyDeviceToHost, ctx->stream));
    return POLS_OK;
}

// An influence call's tables, BEFORE K7 runs: K7 leaves the side-car RSS of every group in sa->rss (the head of Work::InflGroup; the group
// stage's five values per group follow, then -- f32 batches -- the refinement's X~'e~ per segment / group), Work::InflPrep takes K7r's
// prepare launch.
static int influence_tables(pols_ctx *ctx, const pols_batch *b, StatsArgs *sa, Fit *f) {
    const size_t G = (size_t)b->n_groups;
    int rc;
    void *ip = nullptr, *ig = nullptr;
    if ((rc = ensure_scratch(ctx, Work::InflPrep, round256(sizeof(double) * G * k7r_prep_stride(sa->kt)), &ip))) return rc;
    if ((rc = ensure_scratch(ctx, Work::InflGroup, round256(sizeof(double) * (G * 5 + (b->dtype == POLS_F32 ? seg_items(*sa) * (size_t)sa->kt : 0))), &ig))) return rc;
    sa->rss = static_cast<double *>(ig);
    f->infl_prep = static_cast<double *>(ip);
    f->infl_grp = static_cast<double *>(ig) + G;
    return POLS_OK;
}

// The group stage of K7i, AFTER K7: A^-1 / b / trace / ok by K7r's prepare launch, sigma^2 / df / t_crit per group.
static int influence_group_stage(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_influence_params *q, const StatsArgs &sa,
                                 const Fit &f) {
    const size_t G = (size_t)b->n_groups;
    int rc;
    RobustArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    ra.s = sa;
    ra.prep = f.infl_prep;
    if ((rc = k7r_prepare_launch(ctx, b->dtype, ra))) return rc;
    InflGroupArgs ga;
    std::memset(&ga, 0, sizeof(ga));
    if (b->dtype == POLS_F32) {
        // the Gram matrix of an f32 batch carries f32-sized errors: one step of iterative refinement of b in f64 (k7i_influence.hip)
        ra.part = f.infl_grp + 4 * G;
        if ((rc = k7i_refine_launch(ctx, b->dtype, ra))) return rc;
        ga.xe = ra.part;
        ga.seg_first = sa.seg_offs ? sa.seg_first : nullptr;
    }
    ga.offs = f.d_offs; ga.n_groups = b->n_groups; ga.kt = sa.kt;
    ga.lambda = p->alpha; ga.level = q->level;
    ga.prep = f.infl_prep; ga.rss = sa.rss; ga.grp = f.infl_grp;
    return k7i_group_launch(ctx, ga);
}

// The level that never sees a null: solve, Gram matrices, K7 and what the kind adds, everything left on the device (fit_home copies a host
// batch's outputs back).  An influence call's row pass is the caller's: it owns the rows the diagnostics are for.
// Work::Tables: the coefficients' room serves a device batch whose caller did not ask for them, the six arrays' a host batch
static int statistics_fit(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const StatsCall &call, const pols_out *o,
                          const pols_stats_out *s, Fit *f) {
    const int kt = b->n_features + (b->add_intercept ? 1 : 0);
    if (kt > K7_KMAX) return stats_wide(ctx, b, p, o, s, kt, f);
    const bool host = b->mem == POLS_MEM_HOST;
    const size_t G = (size_t)b->n_groups;
    int rc;
    void *spare = nullptr;
    f->six = SixOut(s, G, kt);
    Carve cv;
    cv.keep(spare, dtype_size(b->dtype) * G * kt);
    f->six.stage(cv, host);
    if ((rc = carve(ctx, Work::Tables, cv))) return rc;
    f->coef.ask(o, host, spare);
    LsInfo info;
    if ((rc = ls_core(ctx, b, p, &f->coef.oo, &info))) return rc;
    f->st = std::move(info.st); f->d_offs = info.d_offs;
    double *gram = nullptr;
    if ((rc = stats_gram(ctx, b, kt, *f, info.gram, &gram))) return rc;
    StatsArgs sa;
    if ((rc = stats_args(ctx, b, p, kt, gram, &sa, f))) return rc;
    if (call.infl() && (rc = influence_tables(ctx, b, &sa, f))) return rc;      // (sets sa.rss: before any copy of sa is taken)
    switch (call.kind) {
        case StatsKind::Robust: rc = run_robust(ctx, b, call.cov(), sa); break;
        case StatsKind::Cluster: rc = run_cluster(ctx, b, call.cl(), sa); break;
        default: rc = run_plain(ctx, b, sa); break;
    }
    if (rc) return rc;
    return call.infl() ? influence_group_stage(ctx, b, p, call.infl(), sa, *f) : POLS_OK;
}

// A host batch's outputs of the fit level: the six arrays, then coefficients / predictions / residuals / status and the call's one
// hipStreamSynchronize (unstage_outputs).  Nothing for a device batch.
static int fit_home(pols_ctx *ctx, const pols_batch *b, Fit *f) {
    if (b->mem != POLS_MEM_HOST) return POLS_OK;
    int rc = f->six.copy_home(ctx);
    return rc ? rc : f->coef.home(ctx, b, b->n_features + (b->add_intercept ? 1 : 0), f->st);
}

// ------------------------------------------------------------------ the null-policy level
// Cluster ids follow their rows: the source row of every kept row (the compaction's own slab bases), then a gather into Work::ClusterCompact;
// *cc is the call's cluster block for the compacted batch (a host batch's counts land in Work::ClusterCounts).
static int compacted_cluster_ids(pols_ctx *ctx, const pols_batch *b, const pols_cluster_params *cl, const Compacted &c, pols_cluster_params *cc) {
    *cc = *cl;
    const size_t G = (size_t)b->n_groups;
    const int ways = cluster_ways(cl);
    int rc;
    const int64_t *src[2] = {nullptr, nullptr};
    if ((rc = cluster_device_ids(ctx, b, cl, ways, src))) return rc;
    const int64_t nv = c.offs[G];
    const size_t colb = round256(sizeof(int64_t) * (size_t)std::max<int64_t>(nv, 1));
    int32_t *map = nullptr;
    int64_t *ids = nullptr, *dst[2] = {nullptr, nullptr};
    Carve cv;
    cv.add(map, sizeof(int32_t) * (size_t)std::max<int64_t>(nv, 1));
    cv.add(ids, colb * (size_t)ways);
    if ((rc = carve(ctx, Work::ClusterCompact, cv))) return rc;
    for (int w = 0; w < ways; ++w) dst[w] = column(ids, colb, (size_t)w);
    if (nv > 0) {
        RowCompactArgs ra = c.ra;
        ra.src = map;
        if ((rc = row_compact_srcmap_launch(ctx, ra))) return rc;
        if ((rc = k7c_gather_ids_launch(ctx, ra.src, nv, src, dst, ways))) return rc;
    }
    for (int w = 0; w < ways; ++w) cc->ids[w] = dst[w];
    if (b->mem == POLS_MEM_HOST && cl->n_clusters) {
        void *nc = nullptr;
        if ((rc = ensure_scratch(ctx, Work::ClusterCounts, round256(sizeof(int64_t) * G * (size_t)ways), &nc))) return rc;
        cc->n_clusters = static_cast<int64_t *>(nc);
    }
    return POLS_OK;
}

// The influence row pass over the ORIGINAL rows (c.st), the compaction's validity bytes telling the fitted rows from the others.  The fit
// uploaded the COMPACTED offsets: the original ones go up again (ctx->offs_id, offs_max_rows and the segment cache's key change with them),
// and the segment tables are those of the original frame.
static int influence_rows_of_frame(pols_ctx *ctx, const pols_batch *b, const Compacted &c, const pols_influence_out *io, const Fit &f) {
    const int64_t *d_offs = nullptr;
    int64_t mr = 0;
    int rc = upload_offsets(ctx, b->group_offsets, b->n_groups, &d_offs, &mr, b->offsets_generation);
    if (rc) return rc;
    SegTables sg;
    if ((rc = ensure_segments(ctx, b, mr, 0, &sg))) return rc;
    return influence_rows(ctx, b, c.st, d_offs, sg, c.vbytes, c.ra.zero_fill, io, f);
}

// The statistics are those of the rows handle_nulls leaves (src/expressions.rs:469-471): filter / zero-fill on the device, then the fit level
// on the filtered batch -- a device batch without nulls (compact_nulls: null_free = 1, valid = nullptr), so the fit level is entered exactly
// once and with null_policy = ignore.  Outputs are per group: a device batch's land where the caller wants them, a host batch's are staged
// in Work::CompactOut and copied home here.  (The compacted batch passes check_batch by
// construction: the caller's batch did, and its offsets start at 0 and end at its row count.)
static int statistics_filtered(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const StatsCall &call, const pols_out *o,
                               const pols_stats_out *s) {
    const bool host = b->mem == POLS_MEM_HOST;
    const int kt = b->n_features + (b->add_intercept ? 1 : 0);
    const size_t G = (size_t)b->n_groups, sz = dtype_size(b->dtype);
    int rc;
    Compacted c;
    if ((rc = compact_nulls(ctx, b, p->null_policy, &c))) return rc;
    pols_ols_params pp = *p;
    pp.null_policy = POLS_NULL_IGNORE;
    StatsCall cc = call;
    pols_cluster_params ccl;
    if (call.cl()) {
        if ((rc = compacted_cluster_ids(ctx, b, call.cl(), c, &ccl))) return rc;
        cc.params = &ccl;
    }
    pols_out od = *o;
    SixOut six(s, G, kt);
    if (host) {
        std::memset(&od, 0, sizeof(od));
        Carve cv;
        cv.keep(od.coef, sz * G * kt, o->coef != nullptr);
        cv.keep(od.status, sizeof(int32_t) * G, o->status != nullptr);
        six.stage(cv, true);
        if ((rc = carve(ctx, Work::CompactOut, cv))) return rc;
    }
    const pols_stats_out sd = six.on_device();
    Fit f;      // (of a device batch: nothing of it is to be copied home)
    if ((rc = statistics_fit(ctx, &c.bb, &pp, cc, &od, &sd, &f))) return rc;
    if (call.infl() && (rc = influence_rows_of_frame(ctx, b, c, call.rows, f))) return rc;
    if (!host) return POLS_OK;
    if (call.cl() && call.cl()->n_clusters)
        POLS_HIP(hipMemcpyAsync(call.cl()->n_clusters, ccl.n_clusters, sizeof(int64_t) * G * (size_t)cluster_ways(call.cl()), hipMemcpyDeviceToHost, ctx->stream));
    if (o->coef) POLS_HIP(hipMemcpyAsync(o->coef, od.coef, sz * G * kt, hipMemcpyDeviceToHost, ctx->stream));
    if (o->status) POLS_HIP(hipMemcpyAsync(o->status, od.status, sizeof(int32_t) * G, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = six.copy_home(ctx))) return rc;
    POLS_HIP(hipStreamSynchronize(ctx->stream));
    return POLS_OK;
}

// ------------------------------------------------------------------ the body of the four entries
static int statistics_run(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const StatsCall &call, pols_out *o, const pols_stats_out *s) {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if ((rc = check_batch(b, o, K8_KMAX))) return rc;
    if (!p || !s) return fail(POLS_ERR_INVALID, "params / stats is NULL");
    if (p->null_policy < POLS_NULL_IGNORE || p->null_policy > POLS_NULL_DROP_WINDOW) return fail(POLS_ERR_INVALID, "unknown null_policy %d", p->null_policy);
    if (b->valid && (p->null_policy == POLS_NULL_IGNORE || p->null_policy == POLS_NULL_ZERO))
        return fail(POLS_ERR_INVALID, "a validity mask needs a drop-family null_policy");
    if (b->n_groups == 0) return POLS_OK;
    if ((p->null_policy != POLS_NULL_IGNORE && !b->null_free) || b->valid) return statistics_filtered(ctx, b, p, call, o, s);
    Fit f;
    if ((rc = statistics_fit(ctx, b, p, call, o, s, &f))) return rc;
    if (call.infl() && (rc = influence_rows(ctx, b, f.st, f.d_offs, f.sg, nullptr, 0, call.rows, f))) return rc;
    return fit_home(ctx, b, &f);
}

}  // namespace pols

using namespace pols;

extern "C" {

int pols_least_squares_statistics(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, pols_out *o,
                                  const pols_stats_out *s) {
    return statistics_run(ctx, b, p, StatsCall(), o, s);
}

void pols_cov_params_default(pols_cov_params *c) {
    if (!c) return;
    c->cov_type = POLS_COV_NONROBUST;
    c->maxlags = 0;
}

int pols_least_squares_statistics_robust(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_cov_params *cov,
                                         pols_out *o, const pols_stats_out *s) {
    if (!cov) return fail(POLS_ERR_INVALID, "cov is NULL");
    if (cov->cov_type == POLS_COV_CLUSTER || cov->cov_type == POLS_COV_CLUSTER2)
        return fail(POLS_ERR_INVALID, "cov_type %d: cluster-robust standard errors go through pols_least_squares_statistics_cluster", cov->cov_type);
    if (cov->cov_type < POLS_COV_NONROBUST || cov->cov_type > POLS_COV_HAC) return fail(POLS_ERR_INVALID, "unknown cov_type %d", cov->cov_type);
    if (cov->cov_type == POLS_COV_NONROBUST) return pols_least_squares_statistics(ctx, b, p, o, s);
    if (cov->cov_type == POLS_COV_HAC) {
        if (cov->maxlags < 0) return fail(POLS_ERR_INVALID, "HAC: maxlags %d < 0", cov->maxlags);
        if (cov->maxlags > K7R_MAXLAGS) return fail(POLS_ERR_UNSUPPORTED, "HAC: maxlags %d > %d", cov->maxlags, K7R_MAXLAGS);
    }
    if (!b) return fail(POLS_ERR_INVALID, "batch is NULL");
    const int kt = b->n_features + (b->add_intercept ? 1 : 0);
    if (kt > K7_KMAX)
        return fail(POLS_ERR_UNSUPPORTED, "robust statistics: %d features (incl. intercept) > %d; wider frames have only the non-robust form", kt, K7_KMAX);
    StatsCall call;
    call.kind = StatsKind::Robust; call.params = cov;
    return statistics_run(ctx, b, p, call, o, s);
}

void pols_influence_params_default(pols_influence_params *q) {
    if (!q) return;
    q->level = 0.95;
}

int pols_least_squares_influence(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_influence_params *q,
                                 pols_out *o, const pols_influence_out *infl) {
    if (!q || !infl) return fail(POLS_ERR_INVALID, "influence params / outputs are NULL");
    if (!(q->level > 0.0 && q->level < 1.0)) return fail(POLS_ERR_INVALID, "influence: level %g outside (0, 1)", q->level);
    if (!b) return fail(POLS_ERR_INVALID, "batch is NULL");
    const int kt = b->n_features + (b->add_intercept ? 1 : 0);
    if (kt > K7_KMAX)
        return fail(POLS_ERR_UNSUPPORTED, "influence: %d features (incl. intercept) > %d; wider frames have only the statistics", kt, K7_KMAX);
    pols_stats_out none;
    std::memset(&none, 0, sizeof(none));
    StatsCall call;
    call.kind = StatsKind::Influence; call.params = q; call.rows = infl;
    return statistics_run(ctx, b, p, call, o, &none);
}

void pols_cluster_params_default(pols_cluster_params *c) {
    if (!c) return;
    c->cov_type = POLS_COV_CLUSTER;
    c->use_correction = 1;
    c->ids[0] = c->ids[1] = nullptr;
    c->n_clusters = nullptr;
}

int pols_least_squares_statistics_cluster(pols_ctx *ctx, const pols_batch *b, const pols_ols_params *p, const pols_cluster_params *cl,
                                          pols_out *o, const pols_stats_out *s) {
    if (!cl) return fail(POLS_ERR_INVALID, "cluster params are NULL");
    if (cl->cov_type != POLS_COV_CLUSTER && cl->cov_type != POLS_COV_CLUSTER2)
        return fail(POLS_ERR_INVALID, "cluster statistics: cov_type %d is neither POLS_COV_CLUSTER nor POLS_COV_CLUSTER2", cl->cov_type);
    if (!b) return fail(POLS_ERR_INVALID, "batch is NULL");
    const int kt = b->n_features + (b->add_intercept ? 1 : 0);
    if (kt > K7_KMAX)
        return fail(POLS_ERR_UNSUPPORTED, "cluster statistics: %d features (incl. intercept) > %d; wider frames have only the non-robust form", kt, K7_KMAX);
    const int ways = cluster_ways(cl);
    for (int w = 0; w < ways; ++w)
        if (!cl->ids[w] && b->n_rows > 0) return fail(POLS_ERR_INVALID, "cluster statistics: ids[%d] is NULL", w);
    if (b->n_rows >= ((int64_t)1 << 31)) return fail(POLS_ERR_UNSUPPORTED, "cluster statistics: %lld rows (row indices are 31-bit)", (long long)b->n_rows);
    StatsCall call;
    call.kind = StatsKind::Cluster; call.params = cl;
    return statistics_run(ctx, b, p, call, o, s);
}

}  // extern "C"
