// api.hip -- C-ABI entry points of libpols_mi355x.so (see include/pols_mi355x.h).
#include <algorithm>
#include <cmath>
#include <cctype>
#include <cstdlib>
#include <strings.h>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "common.hpp"
#include "api_internal.hpp"
#include "k1_gram_chol.hpp"
#include "k2_resident.hpp"
#include "k2w_resident.hpp"
#include "k4_rolling.hpp"
#include "k5_enet.hpp"
#include "k6_svd.hpp"
#include "k8_wide.hpp"
#include "k10_ridge_path.hpp"
#include "k11_rlm.hpp"
#include "k13_glm.hpp"
#include "k14_iv.hpp"
#include "k12_enet_cv.hpp"
#include "dyn_prep.hpp"

namespace pols {
template <typename T> bool k1m_fits(int k_user, bool has_w, int64_t max_rows);   // k1m_f32.hip / k1m_f64.hip

// solve_ridge_svd with a caller-supplied rcond (ls.rs:143-148) truncates singular values on EVERY group, so every non-empty group
// is handed to the Jacobi-SVD pass: its status word becomes POLS_GROUP_FALLBACK and the call's epoch is published.
__global__ void __launch_bounds__(256) mark_fallback_kernel(const int64_t *offs, int64_t n_groups, int32_t *status, int32_t *fb_flag,
                                                            int32_t epoch, int only_if_not_empty) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g == 0) *fb_flag = epoch;
    if (g >= n_groups) return;
    if (only_if_not_empty) { if (status[g] != POLS_GROUP_EMPTY) status[g] = POLS_GROUP_FALLBACK; }
    else status[g] = POLS_GROUP_FALLBACK;     // empty groups too: the SVD pass writes their zero coefficients and marks them EMPTY
    (void)offs;
}

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ------------------------------------------------------------------ scratch / offsets / timing
int grow(DeviceBuffer &b, size_t bytes, void **out, bool *fresh) {
    if (fresh) *fresh = bytes > b.cap;
    if (bytes > b.cap) {
        if (b.ptr) POLS_HIP(hipFree(b.ptr));
        b.ptr = nullptr;
        b.cap = 0;
        const size_t want = std::max(bytes, (size_t)1 << 16);
        POLS_HIP(hipMalloc(&b.ptr, want));
        b.cap = want;
    }
    *out = b.ptr;
    return POLS_OK;
}
int grow(CachedTable &t, size_t bytes, void **out) {
    if (bytes > t.buf.cap) t.valid = false;
    return grow(t.buf, bytes, out);
}
int ensure_scratch(pols_ctx *ctx, Work w, size_t bytes, void **out) { return grow(ctx->work[(int)w], bytes, out); }

int upload_small(pols_ctx *ctx, void *dst_device, const void *src, size_t bytes) {
    if (bytes == 0) return POLS_OK;
    if (bytes > ((size_t)1 << 20)) {
        // not small (per-row tables of a masked frame, offsets of millions of groups): straight from the caller's array, and the
        // stream is drained before returning because `src` may be freed -- the pinned ring stays at ~1 MB per slot for good
        POLS_HIP(hipMemcpyAsync(dst_device, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        POLS_HIP(hipStreamSynchronize(ctx->stream));
        return POLS_OK;
    }
    auto &slot = ctx->pinned[ctx->pinned_next];
    ctx->pinned_next = (ctx->pinned_next + 1) % 4;
    if (slot.busy) { POLS_HIP(hipEventSynchronize(slot.done)); slot.busy = false; }   // long complete in steady state
    if (bytes > slot.cap) {
        if (slot.ptr) POLS_HIP(hipHostFree(slot.ptr));
        slot.ptr = nullptr; slot.cap = 0;
        const size_t want = std::max(bytes, (size_t)1 << 16);
        POLS_HIP(hipHostMalloc(&slot.ptr, want, hipHostMallocDefault));
        slot.cap = want;
    }
    if (!slot.done) POLS_HIP(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    std::memcpy(slot.ptr, src, bytes);
    POLS_HIP(hipMemcpyAsync(dst_device, slot.ptr, bytes, hipMemcpyHostToDevice, ctx->stream));
    POLS_HIP(hipEventRecord(slot.done, ctx->stream));
    slot.busy = true;
    return POLS_OK;
}

// One pass over the host offsets: the statistics the dispatchers read (largest group, alignment, size histogram, overflow rows).
bool scan_offsets(const int64_t *offs, int64_t n_groups, OffsetsScan *s) {
    const int64_t cnt = n_groups + 1;
    *s = OffsetsScan();
    int64_t mx = 0, ored = 0, mn = 0, mn_pos = INT64_MAX;
    for (int64_t i = 0; i < cnt; ++i) ored |= offs[i];
    for (int64_t i = 1; i < cnt; ++i) {
        const int64_t d = offs[i] - offs[i - 1];
        mn = d < mn ? d : mn; mx = d > mx ? d : mx;
        mn_pos = (d > 0 && d < mn_pos) ? d : mn_pos;
        s->wave_overflow += d > 1021 ? d - 1021 : 0;
        if (d > 0 && d <= 32) s->small_mask |= d <= 4 ? 1 : (d <= 8 ? 2 : (d <= 16 ? 4 : 8));
        const int bkt = d <= 1 ? 0 : 64 - __builtin_clzll((unsigned long long)(d - 1));
        s->hist_cnt[bkt < 47 ? bkt : 47]++; s->hist_rows[bkt < 47 ? bkt : 47] += d;
    }
    if (mn < 0) return false;
    s->max_rows = mx;
    s->min_rows = mn_pos == INT64_MAX ? 0 : mn_pos;
    for (int64_t i = n_groups; i >= 1; --i)
        if (offs[i] > offs[i - 1]) { s->tail_group = i - 1; break; }
    s->aligned[0] = (ored & 1) == 0;
    s->aligned[1] = (ored & 3) == 0;
    return true;
}

int upload_offsets(pols_ctx *ctx, const int64_t *offs, int64_t n_groups, const int64_t **d_offs, int64_t *max_rows,
                   uint64_t generation) {
    const int64_t cnt = n_groups + 1;
    const size_t bytes = sizeof(int64_t) * (size_t)cnt;
    // Promised hit: the caller vouches that (pointer, count, generation) names the same content as last time -- O(1), what a
    // marshalled Plan passes.  The statistics of the offsets (largest group, alignment, overflow rows) are cached with them.
    if (generation != 0 && ctx->offsets.valid && ctx->offs_host == offs && ctx->offs_n == n_groups &&
        ctx->offs_generation == generation) {
        *d_offs = static_cast<const int64_t *>(ctx->offsets.buf.ptr);
        *max_rows = ctx->offs_max_rows;
        return POLS_OK;
    }
    // Otherwise the content decides.  A cheap hash (four independent multiply-xor chains) picks the candidate, a memcmp
    // against the host copy of what was uploaded CONFIRMS it: a collision can never make two frames share offsets.
    uint64_t h0 = 1469598103934665603ULL, h1 = 0x9E3779B97F4A7C15ULL, h2 = 0xC2B2AE3D27D4EB4FULL, h3 = 0x165667B19E3779F9ULL;
    const uint64_t P = 1099511628211ULL;
    const uint64_t *u = reinterpret_cast<const uint64_t *>(offs);
    int64_t g = 0;
    for (; g + 4 <= cnt; g += 4) {
        h0 = (h0 ^ u[g]) * P; h1 = (h1 ^ u[g + 1]) * P; h2 = (h2 ^ u[g + 2]) * P; h3 = (h3 ^ u[g + 3]) * P;
    }
    for (; g < cnt; ++g) h0 = (h0 ^ u[g]) * P;
    OffsetsScan sc;
    if (!scan_offsets(offs, n_groups, &sc)) return fail(POLS_ERR_INVALID, "group_offsets must be ascending");
    const uint64_t sum = ((h0 * 31 + h1) * 31 + h2) * 31 + h3;
    const bool hit = ctx->offsets.valid && ctx->offs_n == n_groups && ctx->offs_sum == sum &&
                     ctx->offs_copy.size() == (size_t)cnt && std::memcmp(ctx->offs_copy.data(), offs, bytes) == 0;
    if (!hit) {
        void *dptr = nullptr;
        ctx->offsets.valid = false;
        int rc = grow(ctx->offsets, bytes, &dptr);
        if (rc) return rc;
        if ((rc = upload_small(ctx, dptr, offs, bytes))) return rc;   // pinned ring: no stream synchronisation
        ctx->offsets.valid = true;
        ctx->offs_copy.assign(offs, offs + cnt);
        ctx->offs_n = n_groups;
        ctx->offs_sum = sum;
        ctx->offs_id++;
    }
    ctx->offs_host = offs;
    ctx->offs_generation = generation;
    ctx->offs_max_rows = sc.max_rows;
    ctx->offs_min_rows = sc.min_rows;
    ctx->offs_small_mask = sc.small_mask;
    std::memcpy(ctx->offs_hist_cnt, sc.hist_cnt, sizeof(sc.hist_cnt));
    std::memcpy(ctx->offs_hist_rows, sc.hist_rows, sizeof(sc.hist_rows));
    ctx->offs_wave_overflow = sc.wave_overflow;
    ctx->offs_tail_group = sc.tail_group;
    ctx->offs_aligned[0] = sc.aligned[0];
    ctx->offs_aligned[1] = sc.aligned[1];
    *d_offs = static_cast<const int64_t *>(ctx->offsets.buf.ptr);
    *max_rows = sc.max_rows;
    return POLS_OK;
}

// ------------------------------------------------------------------ options (POLS_* knobs)
static bool ieq(const char *a, const char *b) {
    for (; *a && *b; ++a, ++b)
        if (std::tolower((unsigned char)*a) != std::tolower((unsigned char)*b)) return false;
    return *a == *b;
}

bool options_set(Options &o, const char *key, const char *v) {
    if (!key) return false;
    if (!strncasecmp(key, "POLS_", 5)) key += 5;
    const bool on = v != nullptr;
    const Options d;
    if (ieq(key, "TIMELINE")) o.timeline = on;
    else if (ieq(key, "K1_NOOCC4")) o.k1_noocc4 = on;
    else if (ieq(key, "K1_NOFAST")) o.k1_nofast = on;
    else if (ieq(key, "K1_NOEDGE")) o.k1_noedge = on;
    else if (ieq(key, "K1_NOTINY")) o.k1_notiny = on;
    else if (ieq(key, "K1_NORC1")) o.k1_norc1 = on;
    else if (ieq(key, "K1_SHAPE")) { o.k1_shape_team = on && ieq(v, "team"); o.k1_shape_wave = on && ieq(v, "wave"); }
    else if (ieq(key, "K1_F64_TEAM")) o.k1_f64_team256 = on && std::atoi(v) == 256;
    else if (ieq(key, "KG_NOYV")) o.kg_noyv = on;
    else if (ieq(key, "KG_SINGLE_BUFFER")) o.kg_single_buffer = on;
    else if (ieq(key, "NO_CLASSES")) o.no_classes = on;
    else if (ieq(key, "PREDICT_LOOP")) o.predict_loop = on;
    else if (ieq(key, "K2_NOPREFETCH")) o.k2_noprefetch = on;
    else if (ieq(key, "NO_SPLIT")) o.no_split = on;
    else if (ieq(key, "K1_PASSES")) o.k1_passes = on ? std::atoi(v) : d.k1_passes;
    else if (ieq(key, "K1_WG")) o.k1_wg = on ? std::atoi(v) : d.k1_wg;
    else if (ieq(key, "K1T_RC4")) o.k1t_rc4 = on ? (std::atoi(v) != 0) : d.k1t_rc4;
    else if (ieq(key, "K1T_SUB8")) o.k1t_sub8 = on ? std::atoi(v) : d.k1t_sub8;
    else if (ieq(key, "K1_NT_LOADS")) o.k1_nt_loads = on ? (std::atoi(v) != 0) : d.k1_nt_loads;
    else if (ieq(key, "K1_XCD")) o.k1_xcd = on ? std::atoi(v) : d.k1_xcd;
    else if (ieq(key, "K4P_LPS")) o.k4p_lps = on ? std::atoi(v) : d.k4p_lps;
    else if (ieq(key, "SEG_TARGET")) o.seg_target = on ? std::atoi(v) : d.seg_target;
    else if (ieq(key, "K1_RC2_WIDE")) o.k1_rc2_wide = on ? std::atoi(v) != 0 : d.k1_rc2_wide;
    else if (ieq(key, "DEBUG_SKIP_FIXUP")) o.debug_skip_fixup = on && std::atoi(v) != 0;
    else if (ieq(key, "K1_PERSIST")) o.k1_persist = on ? (std::atoi(v) != 0) : d.k1_persist;
    else if (ieq(key, "K1_PERSIST_SUB")) o.k1_persist_sub = on ? std::atoi(v) : d.k1_persist_sub;
    else if (ieq(key, "K1T_SUB32")) o.k1t_sub32 = on ? (std::atoi(v) != 0) : d.k1t_sub32;
    else if (ieq(key, "STATIC_ENGINE")) o.static_engine = !on ? 0 : ieq(v, "stream") ? 1 : ieq(v, "k2") ? 2 : ieq(v, "nok2") ? 3 : ieq(v, "k2w") ? 4 : 0;
    else if (ieq(key, "RLS_ENGINE")) o.rls_engine = !on ? RlsEngine::Auto : ieq(v, "seq") ? RlsEngine::Seq : ieq(v, "scan") ? RlsEngine::Scan : ieq(v, "chunk") ? RlsEngine::Chunk : ieq(v, "halo") ? RlsEngine::Halo : RlsEngine::Auto;
    else if (ieq(key, "RLM_ENGINE")) o.rlm_engine = !on ? 0 : ieq(v, "stream") ? 1 : 0;
    else if (ieq(key, "GLM_ENGINE")) o.glm_engine = !on ? 0 : ieq(v, "split") ? 1 : 0;
    else if (ieq(key, "ABSORB2_ROUTE")) o.absorb2_route = !on ? 0 : ieq(v, "global") ? 1 : 0;
    else if (ieq(key, "RANDOM_EFFECTS_ROUTE")) o.random_effects_route = !on ? 0 : ieq(v, "global") ? 1 : 0;
    else if (ieq(key, "RLS_SPINS")) o.rls_spin_limit = on ? std::atoi(v) : d.rls_spin_limit;
    else if (ieq(key, "RLS_EARLY")) o.rls_early = on ? std::atoi(v) : d.rls_early;
    else if (ieq(key, "ROLLING_ENGINE")) {
        using E = RollingEngine;
        o.rolling_engine = !on ? E::Auto : ieq(v, "chunk") ? E::Chunk : ieq(v, "halo") ? E::Halo : ieq(v, "nocompact") ? E::NoCompact : ieq(v, "halowave") ? E::HaloWave : ieq(v, "scatter") ? E::Scatter : E::Auto;
    }
    else if (ieq(key, "K1_ENGINE")) o.k1_engine = !on ? 0 : ieq(v, "valu") ? 1 : ieq(v, "mfma") ? 2 : 0;
    else if (ieq(key, "K9_TAKE")) o.k9_take = !on ? 0 : ieq(v, "gather") ? 1 : ieq(v, "scatter") ? 2 : 0;
    else return false;
    return true;
}

void options_from_env(Options &o) {
    static const char *const keys[] = {"TIMELINE", "K1_NOOCC4", "K1_NOFAST", "K1_NOTINY", "K1_NORC1", "K1_SHAPE", "K1_F64_TEAM",
                                       "KG_NOYV", "K2_NOPREFETCH", "K1_PASSES", "K1_WG", "RLS_SPINS", "RLS_EARLY", "K1T_RC4", "K1_NT_LOADS", "STATIC_ENGINE",
                                       "RLS_ENGINE", "RLM_ENGINE", "GLM_ENGINE", "ABSORB2_ROUTE", "RANDOM_EFFECTS_ROUTE", "ROLLING_ENGINE", "K1_ENGINE", "K9_TAKE", "K1_PERSIST", "K1_PERSIST_SUB", "K1T_SUB32", "K1_NOEDGE", "K1T_SUB8",
                                       "K1_XCD", "NO_SPLIT", "DEBUG_SKIP_FIXUP", "K4P_LPS", "SEG_TARGET", "K1_RC2_WIDE", "KG_SINGLE_BUFFER", "PREDICT_LOOP", "NO_CLASSES"};
    char name[64];
    for (const char *k : keys) {
        std::snprintf(name, sizeof(name), "POLS_%s", k);
        if (const char *v = std::getenv(name)) options_set(o, k, v);
    }
}

static bool timing_sampled(pols_ctx *ctx) {           // every timing_stride-th eligible launch is timed
    if (!ctx->timing) return false;
    return (ctx->timing_tick++ % ctx->timing_stride) == 0;
}

void timing_begin(pols_ctx *ctx) {
    ctx->timing_open = false;
    if (!timing_sampled(ctx)) return;
    ctx->timing_open = true;
    if (ctx->timed_used == ctx->timed.size()) {
        TimedLaunch t;
        if (hipEventCreate(&t.start) != hipSuccess || hipEventCreate(&t.stop) != hipSuccess) return;
        ctx->timed.push_back(t);
    }
    hipEventRecord(ctx->timed[ctx->timed_used].start, ctx->stream);
}

bool timing_pair(pols_ctx *ctx, hipEvent_t *start, hipEvent_t *stop) {
    if (!timing_sampled(ctx)) return false;
    if (ctx->timed_used == ctx->timed.size()) {
        TimedLaunch t;
        if (hipEventCreate(&t.start) != hipSuccess || hipEventCreate(&t.stop) != hipSuccess) return false;
        ctx->timed.push_back(t);
    }
    *start = ctx->timed[ctx->timed_used].start;
    *stop = ctx->timed[ctx->timed_used].stop;
    ctx->timed_used++;
    return true;
}

void timing_end(pols_ctx *ctx) {
    if (!ctx->timing_open || ctx->timed_used >= ctx->timed.size()) return;
    ctx->timing_open = false;
    hipEventRecord(ctx->timed[ctx->timed_used].stop, ctx->stream);
    ctx->timed_used++;
}

int check_ctx(pols_ctx *ctx) {
    if (!ctx) return fail(POLS_ERR_INVALID, "ctx is NULL");
    POLS_HIP(hipSetDevice(ctx->device));
    return POLS_OK;
}


// Null sample weights of the static entries: sqrt_w = w.sqrt().fill_null(1e-12) in the reference's Python layer
// (polars_ols/least_squares.py:193) -- a null (NaN) weight acts as the weight 1e-24.  One read + write pass of the weights column,
// 16 bytes per lane; skipped when the batch promises null_free.
template <typename T>
__global__ void __launch_bounds__(256) null_weights_kernel(const T *w, T *out, int64_t n) {
    using V = typename Vec16<T>::type;
    constexpr int VN = Vec16<T>::N;
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VN;
    if (i0 + VN <= n) {
        const V v = *reinterpret_cast<const V *>(w + i0);
        T f[4];
#pragma unroll
        for (int e = 0; e < VN; ++e) { const T x = vget<T>(v, e); f[e] = x != x ? (T)1e-24 : x; }
        if constexpr (VN == 4) *reinterpret_cast<V *>(out + i0) = V{f[0], f[1], f[2], f[3]};
        else *reinterpret_cast<V *>(out + i0) = V{f[0], f[1]};
    } else {
        for (int64_t i = i0; i < n; ++i) { const T x = w[i]; out[i] = x != x ? (T)1e-24 : x; }
    }
}

int fill_null_weights(pols_ctx *ctx, const pols_batch *b, Staged *st) {
    if (!st->w || b->null_free || b->n_rows <= 0) return POLS_OK;
    void *dst = const_cast<void *>(st->w);                     // HOST batch: the staged copy is ours -- in place
    if (b->mem == POLS_MEM_DEVICE) {                           // DEVICE batch: the caller's column stays untouched
        int rc = ensure_scratch(ctx, Work::NullWeights, round256(dtype_size(b->dtype) * (size_t)b->n_rows), &dst);
        if (rc) return rc;
    }
    const int vn = b->dtype == POLS_F32 ? 4 : 2;
    const unsigned blocks = (unsigned)((b->n_rows + 256 * (int64_t)vn - 1) / (256 * (int64_t)vn));
    if (b->dtype == POLS_F32) hipLaunchKernelGGL(null_weights_kernel<float>, dim3(blocks), dim3(256), 0, ctx->stream, static_cast<const float *>(st->w), static_cast<float *>(dst), b->n_rows);
    else hipLaunchKernelGGL(null_weights_kernel<double>, dim3(blocks), dim3(256), 0, ctx->stream, static_cast<const double *>(st->w), static_cast<double *>(dst), b->n_rows);
    POLS_HIP(hipGetLastError());
    st->w = dst;
    return POLS_OK;
}

int stage_inputs(pols_ctx *ctx, const pols_batch *b, int64_t coef_rows, int kt, const pols_out *o, Staged *st) {
    const size_t sz = dtype_size(b->dtype);
    const size_t colb = round256(sz * (size_t)b->n_rows);
    st->x.assign((size_t)b->n_features, nullptr);
    if (b->mem == POLS_MEM_DEVICE) {
        st->y = b->y; st->w = b->weights; st->valid = b->valid;
        for (int j = 0; j < b->n_features; ++j) st->x[j] = b->x_cols[j];
        if (o) { st->coef = o->coef; st->pred = o->pred; st->resid = o->resid; st->status = o->status; }
        bool ok = aligned16(st->y) && aligned16(st->w) && aligned16(st->pred) && aligned16(st->resid);
        for (int j = 0; j < b->n_features; ++j) ok = ok && aligned16(st->x[j]);
        if (!ok) return fail(POLS_ERR_INVALID, "device columns must be 16-byte aligned");
        return POLS_OK;
    }
    // the weights take no room when there are none; the validity bytes keep theirs, so that a frame's buffer does not depend on its nulls
    const void *xs = nullptr;
    Carve in;
    in.keep(st->y, colb);
    in.keep(xs, colb * (size_t)b->n_features);
    if (b->weights) in.keep(st->w, colb);
    in.keep(st->valid, (size_t)b->n_rows, b->valid != nullptr);
    int rc = carve(ctx, Work::HostInputs, in);
    if (rc) return rc;
    auto put = [&](const void *dst, const void *src, size_t bytes) -> int {
        POLS_HIP(hipMemcpyAsync(const_cast<void *>(dst), src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return POLS_OK;
    };
    if ((rc = put(st->y, b->y, sz * b->n_rows))) return rc;
    for (int j = 0; j < b->n_features; ++j)
        if ((rc = put(st->x[j] = column(xs, colb, (size_t)j), b->x_cols[j], sz * b->n_rows))) return rc;
    if (b->weights && (rc = put(st->w, b->weights, sz * b->n_rows))) return rc;
    if (b->valid && (rc = put(st->valid, b->valid, (size_t)b->n_rows))) return rc;
    if (o) {
        // a slot the caller does not want stays nullptr; its room stays, so that what is wanted does not move the others
        Carve out;
        out.keep(st->coef, sz * (size_t)coef_rows * kt, o->coef != nullptr);
        out.keep(st->pred, colb, o->pred != nullptr);
        out.keep(st->resid, colb, o->resid != nullptr);
        out.keep(st->status, sizeof(int32_t) * (size_t)b->n_groups, o->status != nullptr);
        if ((rc = carve(ctx, Work::HostOutputs, out))) return rc;
    }
    return POLS_OK;
}

int unstage_outputs(pols_ctx *ctx, const pols_batch *b, int64_t coef_rows, int kt, const pols_out *o, const Staged &st) {
    if (b->mem == POLS_MEM_DEVICE) return POLS_OK;
    const size_t sz = dtype_size(b->dtype);
    if (o->coef) POLS_HIP(hipMemcpyAsync(o->coef, st.coef, sz * (size_t)coef_rows * kt, hipMemcpyDeviceToHost, ctx->stream));
    if (o->pred) POLS_HIP(hipMemcpyAsync(o->pred, st.pred, sz * (size_t)b->n_rows, hipMemcpyDeviceToHost, ctx->stream));
    if (o->resid) POLS_HIP(hipMemcpyAsync(o->resid, st.resid, sz * (size_t)b->n_rows, hipMemcpyDeviceToHost, ctx->stream));
    if (o->status) POLS_HIP(hipMemcpyAsync(o->status, st.status, sizeof(int32_t) * (size_t)b->n_groups, hipMemcpyDeviceToHost, ctx->stream));
    POLS_HIP(hipStreamSynchronize(ctx->stream));
    return POLS_OK;
}

int check_batch(const pols_batch *b, const pols_out *o, int max_features) {
    if (!b || !o) return fail(POLS_ERR_INVALID, "batch / out is NULL");
    if (b->dtype != POLS_F32 && b->dtype != POLS_F64) return fail(POLS_ERR_INVALID, "dtype must be POLS_F32 or POLS_F64");
    if (b->mem != POLS_MEM_HOST && b->mem != POLS_MEM_DEVICE) return fail(POLS_ERR_INVALID, "mem must be POLS_MEM_HOST or POLS_MEM_DEVICE");
    if (b->n_rows < 0 || b->n_groups < 0) return fail(POLS_ERR_INVALID, "negative size");
    if (b->n_features < 1) return fail(POLS_ERR_INVALID, "must pass at least 2 series");  // ex.rs:72
    if (b->n_features + (b->add_intercept ? 1 : 0) > max_features)
        return fail(POLS_ERR_UNSUPPORTED, "%d features (+ intercept) > %d", b->n_features, max_features);
    if (!b->group_offsets || !b->x_cols || (!b->y && b->n_rows)) return fail(POLS_ERR_INVALID, "NULL column / offsets pointer");
    if (b->group_offsets[0] != 0 || b->group_offsets[b->n_groups] != b->n_rows)
        return fail(POLS_ERR_INVALID, "group_offsets must start at 0 and end at n_rows");
    for (int j = 0; j < b->n_features; ++j)
        if (!b->x_cols[j] && b->n_rows) return fail(POLS_ERR_INVALID, "x_cols[%d] is NULL", j);
    return POLS_OK;
}

// handle_nulls for the entries that work on FILTERED rows (Compacted, api_internal.hpp): slab-parallel compaction inside every group
int compact_nulls(pols_ctx *ctx, const pols_batch *b, int policy, Compacted *c, const void *const *targets, int n_targets) {
    int rc;
    const int64_t *d_offs = nullptr;
    int64_t max_rows = 0;
    Staged &st = c->st;
    if ((rc = upload_offsets(ctx, b->group_offsets, b->n_groups, &d_offs, &max_rows, b->offsets_generation))) return rc;
    if ((rc = stage_inputs(ctx, b, 0, 0, nullptr, &st))) return rc;
    const int m = n_targets > 0 ? n_targets : 1;
    const int k = b->n_features, ncols = m + k + (st.w ? 1 : 0);
    const size_t G = (size_t)b->n_groups, N = (size_t)b->n_rows;
    const size_t sz = dtype_size(b->dtype), colb = round256(sz * std::max<size_t>(N, 1));
    const size_t n_slabs = (N + 255) / 256;
    const bool stage_targets = n_targets > 0 && b->mem == POLS_MEM_HOST;      // host targets: uploaded behind the compacted columns
    // slab-parallel (dyn_prep.hip, 256 rows per workgroup whatever the group sizes -- one long group used to be ONE workgroup's
    // count and scatter): validity bytes, valid rows per slab + scan, the compacted offset of every group, a stable scatter
    RowCompactArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    char *cols = nullptr, *staged = nullptr;
    Carve cv;
    cv.add(ra.slab_cnt, sizeof(uint32_t) * std::max<size_t>(n_slabs, 1));
    cv.add(ra.slab_base, sizeof(int64_t) * (n_slabs + 1));
    cv.add(ra.slab_gfirst, sizeof(int64_t) * std::max<size_t>(n_slabs, 1));
    cv.add(ra.valid_out, std::max<size_t>(N, 1));
    cv.add(ra.in, sizeof(void *) * (size_t)ncols);
    cv.add(ra.out, sizeof(void *) * (size_t)ncols);
    cv.add(ra.c_offs, sizeof(int64_t) * (G + 1));
    cv.add(cols, colb * (size_t)ncols);
    cv.add(staged, stage_targets ? colb * (size_t)m : 0);
    if ((rc = carve(ctx, Work::DynPrep, cv))) return rc;
    std::vector<const void *> inp((size_t)ncols);
    std::vector<void *> outp((size_t)ncols);
    for (int t = 0; t < m; ++t) {
        const void *src = n_targets > 0 ? targets[t] : st.y;
        if (stage_targets) {
            char *dst = column(staged, colb, (size_t)t);
            POLS_HIP(hipMemcpyAsync(dst, targets[t], sz * N, hipMemcpyHostToDevice, ctx->stream));
            src = dst;
        }
        inp[(size_t)t] = src;
    }
    for (int j = 0; j < k; ++j) inp[(size_t)(m + j)] = st.x[(size_t)j];
    if (st.w) inp[(size_t)(m + k)] = st.w;
    for (int j = 0; j < ncols; ++j) outp[(size_t)j] = column(cols, colb, (size_t)j);
    if ((rc = upload_small(ctx, const_cast<void **>(ra.in), inp.data(), sizeof(void *) * (size_t)ncols))) return rc;
    if ((rc = upload_small(ctx, const_cast<void **>(ra.out), outp.data(), sizeof(void *) * (size_t)ncols))) return rc;
    ra.n_cols = ncols;
    ra.w_col = st.w ? m + k : -1;
    ra.drop = (policy == POLS_NULL_DROP || policy == POLS_NULL_DROP_ZERO || policy == POLS_NULL_DROP_WINDOW || policy == POLS_NULL_DROP_Y_ZERO_X) ? 1 : 0;
    ra.n_mask = policy == POLS_NULL_DROP_Y_ZERO_X ? m : m + k;                                 // ex.rs:209-220
    ra.zero_fill = (policy == POLS_NULL_ZERO || policy == POLS_NULL_DROP_Y_ZERO_X) ? 1 : 0;   // ex.rs:264-283
    ra.valid_in = st.valid;
    ra.valid = ra.valid_out;
    ra.offs = d_offs; ra.n_rows = (int64_t)N; ra.n_groups = b->n_groups; ra.n_slabs = (int64_t)n_slabs;
    c->offs.assign(G + 1, 0);
    if (N > 0) {
        if ((rc = row_compact_mask_launch(ctx, b->dtype, ra))) return rc;
        if ((rc = row_compact_offsets_launch(ctx, ra))) return rc;
        POLS_HIP(hipMemcpyAsync(c->offs.data(), ra.c_offs, sizeof(int64_t) * (G + 1), hipMemcpyDeviceToHost, ctx->stream));
        POLS_HIP(hipStreamSynchronize(ctx->stream));       // the compacted offsets are a HOST array of the batch
        if ((rc = row_compact_scatter_launch(ctx, b->dtype, ra))) return rc;
    }
    c->ra = ra;
    c->xcols.assign(outp.begin() + m, outp.begin() + m + k);
    c->ycols.assign(outp.begin(), outp.begin() + m);
    c->d_offs = d_offs;
    c->vbytes = ra.valid_out;
    c->bb = *b;
    c->bb.mem = POLS_MEM_DEVICE;
    c->bb.n_rows = c->offs[G];
    c->bb.group_offsets = c->offs.data();
    c->bb.offsets_generation = 0;
    c->bb.y = outp[0];
    c->bb.x_cols = c->xcols.data();
    c->bb.weights = st.w ? outp[(size_t)(m + k)] : nullptr;
    c->bb.valid = nullptr;
    c->bb.null_free = 1;
    return POLS_OK;
}

}  // namespace pols

using namespace pols;

// Long groups cut into segments: SegTables and what ensure_segments builds are described in api_internal.hpp.
int ensure_segments(pols_ctx *ctx, const pols_batch *b, int64_t max_rows, size_t extra_per_seg, SegTables *t,
                    const std::vector<int32_t> *ids, int64_t class_key) {
    *t = SegTables();
    const int64_t seg_target = ctx->opt.seg_target > 0 ? std::max<int64_t>(256, ctx->opt.seg_target)
                                                      : std::max<int64_t>(4096, ((b->n_rows / std::max<int64_t>(1, 8 * (int64_t)ctx->num_cus) + 1023) / 1024) * 1024);
    if (!ids && (!(max_rows > 2 * seg_target) || ctx->opt.no_split)) return POLS_OK;
    const int64_t n_items = ids ? (int64_t)ids->size() : b->n_groups;
    auto &sc = ctx->seg_cache[ids ? 1 : 0];               // (class tables have their own: they do not evict the whole-frame tables)
    int rc;
    // (the key is the frame; the per-segment extra area only has to be large enough -- its users differ in what they keep there: the Gram
    // partials of ls_core, the moments of the statistics entry, nothing for pols_predict -- and it is kept at the largest size asked for,
    // so that alternating users of one frame stop rebuilding and re-uploading the tables)
    const bool same_frame = sc.valid && sc.offs_id == ctx->offs_id && sc.n_groups == b->n_groups && sc.n_rows == b->n_rows &&
                            sc.seg_target == seg_target && sc.class_key == class_key && sc.n_items == n_items;
    const bool hit = same_frame && sc.nz2 >= extra_per_seg;
    Carve cv;
    if (hit) {
        seg_tables_layout(cv, *t, sc.n_seg, n_items, ids != nullptr, sc.nz2);
        cv.place(sc.buf.ptr);
        t->max_len = sc.max_len; t->max_seg = sc.max_seg;
        return POLS_OK;
    }
    if (same_frame) extra_per_seg = std::max<size_t>(extra_per_seg, sc.nz2);
    sc.valid = false;
    std::vector<int64_t> so;
    std::vector<int32_t> sm, sf((size_t)n_items + 1);
    if (!ids) so.push_back(0);
    int64_t max_len = 0, max_seg = 0;
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t g = ids ? (int64_t)(*ids)[(size_t)i] : i;
        if (i > 0) max_seg = std::max<int64_t>(max_seg, (int64_t)sm.size() - sf[(size_t)i - 1]);
        sf[(size_t)i] = (int32_t)sm.size();
        const int64_t s0 = b->group_offsets[g], e0 = b->group_offsets[g + 1];
        const int64_t pieces = std::max<int64_t>(1, (e0 - s0 + seg_target - 1) / seg_target);
        const int64_t len = std::max<int64_t>(1, ((e0 - s0 + pieces - 1) / pieces + 255) / 256 * 256);   // (256-row multiples: whole staging chunks)
        max_len = std::max(max_len, std::min(len, e0 - s0));
        for (int64_t r = s0; r < e0 || r == s0; r += len) {
            if (ids) so.push_back(r);
            so.push_back(std::min(e0, r + len));
            sm.push_back((int32_t)i);
            if (e0 == s0) break;
        }
    }
    sf[(size_t)n_items] = (int32_t)sm.size();
    if (n_items > 0) max_seg = std::max<int64_t>(max_seg, (int64_t)sm.size() - sf[(size_t)n_items - 1]);
    const int64_t n_seg = (int64_t)sm.size();
    seg_tables_layout(cv, *t, n_seg, n_items, ids != nullptr, extra_per_seg);
    if ((rc = carve(sc, cv))) return rc;
    if ((rc = upload_small(ctx, const_cast<int64_t *>(t->offs), so.data(), sizeof(int64_t) * so.size()))) return rc;
    if ((rc = upload_small(ctx, const_cast<int32_t *>(t->map), sm.data(), sizeof(int32_t) * sm.size()))) return rc;
    if ((rc = upload_small(ctx, const_cast<int32_t *>(t->first), sf.data(), sizeof(int32_t) * sf.size()))) return rc;
    sc.valid = true; sc.offs_id = ctx->offs_id; sc.n_groups = b->n_groups; sc.n_rows = b->n_rows; sc.seg_target = seg_target;
    sc.class_key = class_key; sc.n_items = n_items;
    sc.n_seg = n_seg; sc.nz2 = extra_per_seg; sc.nulls = false; sc.max_len = max_len; sc.max_seg = max_seg;
    t->max_len = max_len; t->max_seg = max_seg;
    return POLS_OK;
}

// ------------------------------------------------------------------ context
extern "C" {

int pols_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *pols_version(void) { return "pols_mi355x 0.1.0 (gfx950)"; }
const char *pols_last_error(void) { return g_err; }

int pols_create(int device_id, pols_ctx **out) {
    if (!out) return fail(POLS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(POLS_ERR_NO_DEVICE, "no HIP device visible; libpols_mi355x has no CPU fallback");
    if (device_id < 0 || device_id >= n) return fail(POLS_ERR_INVALID, "device_id %d out of range [0, %d)", device_id, n);
    POLS_HIP(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    POLS_HIP(hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(POLS_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code objects only", device_id, prop.gcnArchName);
    pols_ctx *ctx = new pols_ctx();
    ctx->device = device_id;
    ctx->num_cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return fail(POLS_ERR_HIP, "hipStreamCreate failed");
    }
    ctx->stream = ctx->own_stream;
    options_from_env(ctx->opt);            // the only getenv calls of the library: no launch path reads the environment
    *out = ctx;
    return POLS_OK;
}

int pols_set_option(pols_ctx *ctx, const char *key, const char *value) {
    if (!ctx || !key) return fail(POLS_ERR_INVALID, "ctx / key is NULL");
    if (!options_set(ctx->opt, key, value)) return fail(POLS_ERR_INVALID, "unknown option '%s'", key);
    return POLS_OK;
}

void pols_destroy(pols_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (DeviceBuffer *d : {&ctx->offsets.buf, &ctx->chunk_cache.buf, &ctx->k3c.buf, &ctx->k3h.buf, &ctx->class_cache.buf, &ctx->seg_cache[0].buf,
                            &ctx->seg_cache[1].buf, &ctx->start_flags.buf, &ctx->k3c_gran, &ctx->k4c_fix})
        if (d->ptr) hipFree(d->ptr);
    for (auto &d : ctx->work)
        if (d.ptr) hipFree(d.ptr);
    if (ctx->fb_flag) hipFree(ctx->fb_flag);
    for (auto &t : ctx->timed) { hipEventDestroy(t.start); hipEventDestroy(t.stop); }
    for (auto &ps : ctx->pinned) {
        if (ps.done) hipEventDestroy(ps.done);
        if (ps.ptr) hipHostFree(ps.ptr);
    }
    if (ctx->switch_event) hipEventDestroy(ctx->switch_event);
    if (ctx->own_stream) hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int pols_set_stream(pols_ctx *ctx, void *hip_stream) {
    if (!ctx) return fail(POLS_ERR_INVALID, "ctx is NULL");
    hipStream_t next = static_cast<hipStream_t>(hip_stream);   // NULL == HIP's null stream (torch's default stream)
    if (next != ctx->stream) {
        // The context's scratch buffers (offsets, Gram matrices, status, staging) are shared by every call: work launched on the
        // new stream must not overtake what is still in flight on the old one.  One event per switch, nothing in steady state.
        if (!ctx->switch_event) POLS_HIP(hipEventCreateWithFlags(&ctx->switch_event, hipEventDisableTiming));
        POLS_HIP(hipEventRecord(ctx->switch_event, ctx->stream));
        POLS_HIP(hipStreamWaitEvent(next, ctx->switch_event, 0));
    }
    ctx->stream = next;
    return POLS_OK;
}

int pols_use_private_stream(pols_ctx *ctx) {
    if (!ctx) return fail(POLS_ERR_INVALID, "ctx is NULL");
    return pols_set_stream(ctx, ctx->own_stream);
}

int pols_synchronize(pols_ctx *ctx) {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    POLS_HIP(hipStreamSynchronize(ctx->stream));
    return POLS_OK;
}

int pols_timing_enable(pols_ctx *ctx, int enable) {
    if (!ctx) return fail(POLS_ERR_INVALID, "ctx is NULL");
    ctx->timing = enable != 0;
    ctx->timing_stride = enable > 1 ? enable : 1;
    ctx->timing_tick = 0;
    ctx->timed_used = 0;
    return POLS_OK;
}

int pols_timing_collect(pols_ctx *ctx, float *ms_out, int max) {
    if (!ctx || !ms_out) return fail(POLS_ERR_INVALID, "NULL argument");
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(POLS_ERR_HIP, "stream sync failed");
    int n = 0;
    for (size_t i = 0; i < ctx->timed_used && n < max; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->timed[i].start, ctx->timed[i].stop) == hipSuccess) ms_out[n++] = ms;
    }
    ctx->timed_used = 0;
    return n;
}

const char *pols_last_kernel_name(pols_ctx *ctx) { return ctx ? ctx->last_kernel.c_str() : ""; }

// ------------------------------------------------------------------ defaults (ls.py:101-107; the dynamic entries': api_dynamic.hip)
void pols_ols_params_default(pols_ols_params *p) {
    std::memset(p, 0, sizeof(*p));
    p->alpha = 0.0;
    p->has_l1_ratio = 0;
    p->max_iter = 1000;
    p->tol = 1.0e-5;
    p->positive = 0;
    p->solve_method = POLS_SOLVE_AUTO;
    p->has_rcond = 0;
    p->null_policy = POLS_NULL_IGNORE;
}

int pols_predict(pols_ctx *ctx, const pols_batch *b, const void *coef, int64_t coef_rows, void *pred_out) {
    return pols_predict_policy(ctx, b, coef, coef_rows, POLS_NULL_IGNORE, pred_out);
}

int pols_predict_policy(pols_ctx *ctx, const pols_batch *b, const void *coef, int64_t coef_rows, int32_t null_policy, void *pred_out) {
    // `predict` plugin body (src/expressions.rs:706-741): sum_j x[t, j] * coef[t, j]; coef in the batch dtype,
    // coef_rows == n_rows (one coefficient row per input row, what Polars broadcasts the struct to).
    int rc = check_ctx(ctx);
    if (rc) return rc;
    pols_out o;
    std::memset(&o, 0, sizeof(o));
    o.pred = pred_out;
    if ((rc = check_batch(b, &o, K8_KMAX))) return rc;
    if (!coef || !pred_out) return fail(POLS_ERR_INVALID, "coef / pred_out is NULL");
    if (coef_rows != b->n_rows) return fail(POLS_ERR_INVALID, "number of coefficient rows must match the number of rows");
    if (b->weights) return fail(POLS_ERR_INVALID, "predict takes no weights");
    if (null_policy != POLS_NULL_IGNORE && null_policy != POLS_NULL_ZERO && null_policy != POLS_NULL_DROP)
        return fail(POLS_ERR_INVALID, "predict: null_policy must be one of ignore / zero / drop (least_squares.py:474)");
    // "zero": nulls (NaNs) in the features count as 0 (ex.rs:725).  "drop" zero-fills too and then nulls the rows with a null anywhere
    // (:732-738): with NaN as the null, that is the un-filled product.
    const int32_t fill_policy = null_policy == POLS_NULL_ZERO ? POLS_NULL_ZERO : POLS_NULL_IGNORE;
    const int kt = b->n_features + (b->add_intercept ? 1 : 0);   // predict adds pl.lit(1.0) for the intercept (ls.py:479-483)
    if (b->n_rows == 0) return POLS_OK;
    const int64_t *d_offs = nullptr;
    int64_t max_rows = 0;
    if ((rc = upload_offsets(ctx, b->group_offsets, b->n_groups, &d_offs, &max_rows, b->offsets_generation))) return rc;
    Staged st;
    if ((rc = stage_inputs(ctx, b, b->n_rows, kt, &o, &st))) return rc;
    const void *d_coef = coef;
    if (b->mem == POLS_MEM_HOST) {
        void *d = nullptr;
        const size_t bytes = dtype_size(b->dtype) * (size_t)coef_rows * kt;
        if ((rc = ensure_scratch(ctx, Work::Gram, bytes, &d))) return rc;
        POLS_HIP(hipMemcpyAsync(d, coef, bytes, hipMemcpyHostToDevice, ctx->stream));
        d_coef = d;
    }
    if (kt > POLS_MAX_FEATURES) {                                  // wide frames: column pointers through a device table
        void *tab = nullptr;
        if ((rc = ensure_scratch(ctx, Work::Tables, sizeof(void *) * (size_t)b->n_features, &tab))) return rc;
        if ((rc = upload_small(ctx, tab, st.x.data(), sizeof(void *) * (size_t)b->n_features))) return rc;
        WideArgs wa;
        std::memset(&wa, 0, sizeof(wa));
        wa.cols = static_cast<const void *const *>(tab);
        wa.n_rows = b->n_rows; wa.k_user = b->n_features; wa.kt = kt; wa.pred = st.pred;
        wa.null_policy = fill_policy;
        ctx->last_kernel = "k8_wide_predict_rows";
        if ((rc = wide_predict_rows_launch(ctx, b->dtype, wa, d_coef))) return rc;
        return unstage_outputs(ctx, b, b->n_rows, kt, &o, st);
    }
    PredictArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    for (int j = 0; j < b->n_features; ++j) pa.x[j] = st.x[j];
    pa.offs = d_offs; pa.n_groups = b->n_groups; pa.n_rows = b->n_rows;
    pa.coef_rows = d_coef; pa.pred = st.pred;
    pa.k_user = b->n_features; pa.kt = kt;
    pa.null_policy = fill_policy;
    ctx->last_kernel = "predict";
    {   // (a group is one workgroup in this kernel: long groups -- the dynamic models' one long sequence -- go segment by segment)
        SegTables sg;
        if ((rc = ensure_segments(ctx, b, max_rows, 0, &sg))) return rc;
        if (sg.n_seg > 0) { pa.offs = sg.offs; pa.n_groups = sg.n_seg; }
        pa.max_item_rows = sg.n_seg > 0 ? sg.max_len : max_rows;
    }
    if ((rc = predict_launch(ctx, b->dtype, pa))) return rc;
    return unstage_outputs(ctx, b, b->n_rows, kt, &o, st);
}

// ------------------------------------------------------------------ one process, several GPUs
// What a Polars plugin process is: ONE process holding the frame in host memory, N devices.  The groups are cut into
// contiguous ranges balanced by rows (pols_partition_groups), range r is solved on ctxs[r]'s device from its own host thread
// (staging over that device's PCIe link, the same kernels, its own stream), and the outputs are re-assembled:
//   out_mem == POLS_MEM_HOST    every device copies its slice straight into the caller's host arrays -- no collective at all;
//   out_mem == POLS_MEM_DEVICE  the outputs are assembled on ctxs[0]'s device over RCCL / xGMI: the per-group coefficient table
//                               with pols_comm_allgather_rows (every device ends up with it; device 0's copy is the caller's
//                               buffer), predictions / residuals / status with pols_comm_gather_rows to device 0 (the root pulls
//                               from its peers over distinct xGMI links).  Each device's collectives are issued by its own thread,
//                               stream-ordered behind its kernels.
int pols_least_squares_sharded(pols_ctx *const *ctxs, pols_comm *const *comms, int n, const pols_batch *b, const pols_ols_params *p,
                               pols_out *o, int32_t out_mem) {
    if (!ctxs || n < 1 || n > 64) return fail(POLS_ERR_INVALID, "ctxs / n");
    if (!b || !p || !o) return fail(POLS_ERR_INVALID, "batch / params / out is NULL");
    if (b->mem != POLS_MEM_HOST) return fail(POLS_ERR_INVALID, "the sharded entry takes a HOST batch (the plugin process holds the frame in host memory)");
    if (out_mem != POLS_MEM_HOST && out_mem != POLS_MEM_DEVICE) return fail(POLS_ERR_INVALID, "out_mem must be POLS_MEM_HOST or POLS_MEM_DEVICE");
    if (out_mem == POLS_MEM_DEVICE && !comms) return fail(POLS_ERR_INVALID, "device-side assembly needs the communicators (pols_comm_create_all)");
    int rc = check_batch(b, o, K8_KMAX);
    if (rc) return rc;
    for (int r = 0; r < n; ++r) {
        if (!ctxs[r]) return fail(POLS_ERR_INVALID, "ctxs[%d] is NULL", r);
        if (out_mem == POLS_MEM_DEVICE && (!comms[r] || pols_comm_world_size(comms[r]) != n || pols_comm_rank(comms[r]) != r))
            return fail(POLS_ERR_INVALID, "comms[%d] is not rank %d of a world of %d", r, r, n);
    }
    const int kt = b->n_features + (b->add_intercept ? 1 : 0);
    const size_t sz = dtype_size(b->dtype);
    std::vector<int64_t> bounds((size_t)n + 1);
    if ((rc = pols_partition_groups(b->group_offsets, b->n_groups, n, bounds.data()))) return rc;
    std::vector<int64_t> gcounts((size_t)n), rcounts((size_t)n);
    for (int r = 0; r < n; ++r) {
        gcounts[(size_t)r] = bounds[(size_t)r + 1] - bounds[(size_t)r];
        rcounts[(size_t)r] = b->group_offsets[bounds[(size_t)r + 1]] - b->group_offsets[bounds[(size_t)r]];
    }
    std::vector<int> rcs((size_t)n, POLS_OK);
    std::vector<std::string> errs((size_t)n);
    // Device-side assembly runs in two phases with a host-side rendezvous between them: a rank that fails BEFORE its collectives
    // (context, scratch, staging copy, solve) must not leave its peers waiting inside RCCL for a send / receive that never comes.
    // Every rank reports after its solve; the collectives are issued only when every rank succeeded.
    std::mutex gate_m;
    std::condition_variable gate_cv;
    int gate_arrived = 0, gate_decision = 0;                       // decision: 0 pending, 1 go, 2 abort
    auto rendezvous = [&]() -> bool {
        std::unique_lock<std::mutex> lk(gate_m);
        ++gate_arrived;
        gate_cv.notify_all();
        gate_cv.wait(lk, [&] { return gate_decision != 0; });
        return gate_decision == 1;
    };
    std::vector<char> met((size_t)n, 0);                           // rank r has been through the rendezvous
    auto work_impl = [&](int r) {
        auto done = [&](int code) {
            rcs[(size_t)r] = code;
            if (code) errs[(size_t)r] = pols_last_error();
            if (out_mem == POLS_MEM_DEVICE && !met[(size_t)r]) { met[(size_t)r] = 1; rendezvous(); }   // a failed rank still reports, so that the others are released
        };
        pols_ctx *ctx = ctxs[r];
        const int64_t g0 = bounds[(size_t)r], g1 = bounds[(size_t)r + 1], row0 = b->group_offsets[g0], nrows = rcounts[(size_t)r];
        // the shard as a batch of its own: column pointers advanced to its first row, offsets rebased to 0
        std::vector<int64_t> offs((size_t)(g1 - g0) + 1);
        for (int64_t g = g0; g <= g1; ++g) offs[(size_t)(g - g0)] = b->group_offsets[g] - row0;
        std::vector<const void *> xs((size_t)b->n_features);
        auto at = [&](const void *base, int64_t row, size_t elem) { return base ? static_cast<const void *>(static_cast<const char *>(base) + (size_t)row * elem) : nullptr; };
        for (int j = 0; j < b->n_features; ++j) xs[(size_t)j] = at(b->x_cols[j], row0, sz);
        pols_batch sb = *b;
        sb.n_rows = nrows; sb.n_groups = g1 - g0; sb.group_offsets = offs.data(); sb.offsets_generation = 0;
        sb.y = at(b->y, row0, sz); sb.x_cols = xs.data(); sb.weights = at(b->weights, row0, sz);
        sb.valid = static_cast<const uint8_t *>(at(b->valid, row0, 1));
        auto out_at = [&](void *base, int64_t row, size_t elem) { return base ? static_cast<void *>(static_cast<char *>(base) + (size_t)row * elem) : nullptr; };
        if (out_mem == POLS_MEM_HOST) {                            // every device writes its own slice of the caller's host arrays
            pols_out so;
            so.coef = out_at(o->coef, g0 * kt, sz); so.pred = out_at(o->pred, row0, sz); so.resid = out_at(o->resid, row0, sz);
            so.status = static_cast<int32_t *>(out_at(o->status, g0, sizeof(int32_t)));
            if (sb.n_groups == 0) return done(POLS_OK);
            return done(pols_least_squares(ctx, &sb, p, &so));
        }
        // device-side assembly: stage the shard on this device (Work::Collective), solve it there with the outputs next to it, then
        // the collectives on this device's stream.  Every rank takes part in every collective, shard or no shard.
        int rc2 = check_ctx(ctx);
        if (rc2) return done(rc2);
        const size_t rows1 = (size_t)std::max<int64_t>(nrows, 1), groups1 = (size_t)std::max<int64_t>(sb.n_groups, 1);
        const size_t colb = round256(sz * rows1);
        pols_batch db = sb;
        db.mem = POLS_MEM_DEVICE;
        pols_out so;
        std::memset(&so, 0, sizeof(so));
        const void *dxs = nullptr;
        void *all_coef = nullptr;
        // the validity bytes and every output keep their room, wanted or not: a rank's buffer depends on the shard's shape alone
        Carve cv;
        cv.keep(db.y, colb, sb.y != nullptr);
        cv.add(dxs, colb * (size_t)b->n_features);
        if (b->weights) cv.add(db.weights, colb);
        cv.keep(db.valid, rows1, b->valid != nullptr);
        cv.keep(so.pred, colb, o->pred != nullptr);
        cv.keep(so.resid, colb, o->resid != nullptr);
        cv.keep(so.coef, sz * groups1 * kt, o->coef != nullptr);
        cv.add(all_coef, sz * (size_t)std::max<int64_t>(b->n_groups, 1) * kt);
        cv.keep(so.status, sizeof(int32_t) * groups1, o->status != nullptr);
        if ((rc2 = carve(ctx, Work::Collective, cv))) return done(rc2);
        auto put = [&](const void *dst, const void *src, size_t bytes) {
            if (src && bytes && hipMemcpyAsync(const_cast<void *>(dst), src, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc2 = POLS_ERR_HIP;
        };
        put(db.y, sb.y, sz * (size_t)nrows);
        std::vector<const void *> dx((size_t)b->n_features);
        for (int j = 0; j < b->n_features; ++j) put(dx[(size_t)j] = column(dxs, colb, (size_t)j), xs[(size_t)j], sz * (size_t)nrows);
        db.x_cols = dx.data();
        if (b->weights) put(db.weights, sb.weights, sz * (size_t)nrows);
        if (b->valid) put(db.valid, sb.valid, (size_t)nrows);
        if (rc2) { set_error("staging copy failed on device %d", ctx->device); return done(rc2); }
        if (sb.n_groups > 0 && (rc2 = pols_least_squares(ctx, &db, p, &so))) return done(rc2);
        met[(size_t)r] = 1;
        if (!rendezvous()) { rcs[(size_t)r] = POLS_OK; return; }    // another rank failed: nobody enters the collectives (its error is reported)
        pols_comm *cm = comms[r];
        if (o->coef && (rc2 = pols_comm_allgather_rows(cm, so.coef, gcounts.data(), (int64_t)(sz * kt), r == 0 ? o->coef : all_coef))) return done(rc2);
        if (o->pred && (rc2 = pols_comm_gather_rows(cm, so.pred, rcounts.data(), (int64_t)sz, 0, r == 0 ? o->pred : nullptr))) return done(rc2);
        if (o->resid && (rc2 = pols_comm_gather_rows(cm, so.resid, rcounts.data(), (int64_t)sz, 0, r == 0 ? o->resid : nullptr))) return done(rc2);
        if (o->status && (rc2 = pols_comm_gather_rows(cm, so.status, gcounts.data(), (int64_t)sizeof(int32_t), 0, r == 0 ? o->status : nullptr))) return done(rc2);
        if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { set_error("stream synchronisation failed on device %d", ctx->device); return done(POLS_ERR_HIP); }
        return done(POLS_OK);
    };
    auto work = [&](int r) {                                       // (an allocation failure inside a device thread must not terminate the process)
        try { work_impl(r); } catch (...) {
            rcs[(size_t)r] = POLS_ERR_INVALID; errs[(size_t)r] = "out of host memory";
            if (out_mem == POLS_MEM_DEVICE && !met[(size_t)r]) { met[(size_t)r] = 1; rendezvous(); }
        }
    };
    {
        std::vector<std::thread> th;
        int started = 0;
        bool all_started = true;
        try {                                                      // no C++ exception may cross the C boundary (thread creation can throw)
            for (; started < n; ++started) th.emplace_back(work, started);
        } catch (...) {
            all_started = false;
        }
        if (out_mem == POLS_MEM_DEVICE) {                          // release the ranks once every started one has reported
            std::unique_lock<std::mutex> lk(gate_m);
            gate_cv.wait(lk, [&] { return gate_arrived == started; });
            bool ok = all_started;
            for (int r = 0; r < started; ++r) ok = ok && rcs[(size_t)r] == POLS_OK;
            gate_decision = ok ? 1 : 2;
            gate_cv.notify_all();
        }
        for (auto &t : th) t.join();
        if (!all_started) return fail(POLS_ERR_INVALID, "could not start the host thread of device %d", started);
    }
    for (int r = 0; r < n; ++r)
        if (rcs[(size_t)r]) return fail(rcs[(size_t)r], "device %d: %s", r, errs[(size_t)r].c_str());
    return POLS_OK;
}

}  // extern "C"

namespace pols {
// the register-resident kernels, a few column counts per translation unit (k1_f32_a.hip ... k1n_f64_b.hip)
#define K1P_DECL(name) int name(pols_ctx *ctx, int kt, const K1Args &a, int64_t max_rows);
K1P_DECL(k1_launch_f32_a) K1P_DECL(k1_launch_f32_b) K1P_DECL(k1_launch_f32_c) K1P_DECL(k1_launch_f64_a) K1P_DECL(k1_launch_f64_b)
K1P_DECL(k1n_launch_f32_a) K1P_DECL(k1n_launch_f32_b) K1P_DECL(k1n_launch_f32_c)   // null-policy family
K1P_DECL(k1n_launch_f64_a) K1P_DECL(k1n_launch_f64_b) K1P_DECL(k1n_launch_f64_c)
#undef K1P_DECL
template <typename T> static int k1_launch_t(pols_ctx *ctx, int kt, const K1Args &a, int64_t max_rows) {
    if constexpr (sizeof(T) == 4) return kt <= 6 ? k1_launch_f32_a(ctx, kt, a, max_rows) : (kt <= 8 ? k1_launch_f32_b(ctx, kt, a, max_rows) : k1_launch_f32_c(ctx, kt, a, max_rows));
    else return kt <= 7 ? k1_launch_f64_a(ctx, kt, a, max_rows) : k1_launch_f64_b(ctx, kt, a, max_rows);
}
template <typename T> static int k1n_launch_t(pols_ctx *ctx, int kt, const K1Args &a, int64_t max_rows) {
    if constexpr (sizeof(T) == 4) return kt <= 7 ? k1n_launch_f32_a(ctx, kt, a, max_rows) : (kt <= 10 ? k1n_launch_f32_b(ctx, kt, a, max_rows) : k1n_launch_f32_c(ctx, kt, a, max_rows));
    else return kt <= 7 ? k1n_launch_f64_a(ctx, kt, a, max_rows) : (kt <= 10 ? k1n_launch_f64_b(ctx, kt, a, max_rows) : k1n_launch_f64_c(ctx, kt, a, max_rows));
}
template <typename T> int k1m_launch_t(pols_ctx *ctx, int kt, const K1Args &a, int64_t max_rows);
// 16..31 columns, resident multi-pass: four column counts per translation unit (k1w_f32_a.hip ... k1w_f64_d.hip)
#define K1W_DECL(name) int name(pols_ctx *ctx, int kt, const K1Args &a, int64_t max_rows);
K1W_DECL(k1w_launch_f32_a) K1W_DECL(k1w_launch_f32_b) K1W_DECL(k1w_launch_f32_c) K1W_DECL(k1w_launch_f32_d)
K1W_DECL(k1w_launch_f64_a) K1W_DECL(k1w_launch_f64_b) K1W_DECL(k1w_launch_f64_c) K1W_DECL(k1w_launch_f64_d)
// ... and their null-policy family (k1nw_*.hip; f64 up to 27 columns: the plain f64 kernels run at 17-24)
K1W_DECL(k1nw_launch_f32_a) K1W_DECL(k1nw_launch_f32_b) K1W_DECL(k1nw_launch_f32_c) K1W_DECL(k1nw_launch_f32_d)
K1W_DECL(k1nw_launch_f64_a) K1W_DECL(k1nw_launch_f64_b) K1W_DECL(k1nw_launch_f64_c)
#undef K1W_DECL

// Engine choice for the static least-squares path:
//   K1m (LDS tile + MFMA Gram)   groups whose tile fits the 160 KiB LDS and are big enough to fill a workgroup;
//   K1  (register-resident VALU)  small groups (one wave per group) and groups too large for LDS (streamed).
// POLS_K1_ENGINE=valu|mfma overrides the choice (A/B measurements).
int k1_launch(pols_ctx *ctx, int dtype, int kt, const K1Args &a, int64_t max_group_rows, bool) {
    const bool f32 = dtype == POLS_F32;
    const int vec = f32 ? 4 : 2;
    if (a.null_policy != POLS_NULL_IGNORE) {
        if (kt > K1X_MAX_KT || (kt > K1W_MAX_KT && !f32 && kt > 27))
            return fail(POLS_ERR_UNSUPPORTED, "k1 null-policy kernels stop at %d columns", f32 ? K1X_MAX_KT : 27);
        if (kt > K1W_MAX_KT) {
            using Fn = int (*)(pols_ctx *, int, const K1Args &, int64_t);
            static const Fn wide[2][4] = {{k1nw_launch_f32_a, k1nw_launch_f32_b, k1nw_launch_f32_c, k1nw_launch_f32_d},
                                          {k1nw_launch_f64_a, k1nw_launch_f64_b, k1nw_launch_f64_c, nullptr}};
            return wide[f32 ? 0 : 1][(kt - 16) / 4](ctx, kt, a, max_group_rows);
        }
        return f32 ? k1n_launch_t<float>(ctx, kt, a, max_group_rows) : k1n_launch_t<double>(ctx, kt, a, max_group_rows);
    }
    const bool fits = kt <= K1M_MAX_KT && (f32 ? k1m_fits<float>(a.k_user, a.w != nullptr, max_group_rows)
                                               : k1m_fits<double>(a.k_user, a.w != nullptr, max_group_rows));
    // Measured on MI355X (10k groups x 1k rows, profiles/r01_*): K1 is at ~90 % of the bandwidth a math-free
    // kernel with the same access pattern reaches whenever a group's rows stay register-resident (k <= 8:
    // <= 2048 rows f32, <= 1024 rows f64); K1m reads HBM once for any group whose tile fits LDS and carries up
    // to 15 features, at ~65 % of that bandwidth (LDS caps it at 4 groups in flight per CU).
    const bool k1_ok = k1_valu_takes(ctx->opt, ctx->offs_aligned[f32 ? 1 : 0], f32, kt, max_group_rows, a.w != nullptr);
    bool use_mfma = fits && !k1_ok && (max_group_rows > 64 * 2 * vec || kt > K1_MAX_KT);
    if (ctx->opt.k1_engine == 1 && kt <= K1_MAX_KT) use_mfma = false;
    if (ctx->opt.k1_engine == 2 && fits) use_mfma = true;
    if (kt > K1_MAX_KT && !k1_ok && !use_mfma)
        return fail(POLS_ERR_UNSUPPORTED, "%d features with %lld-row groups: tile exceeds LDS and the resident engine stops at %d features",
                    kt, (long long)max_group_rows, K1_MAX_KT);
    if (use_mfma) return f32 ? k1m_launch_t<float>(ctx, kt, a, max_group_rows) : k1m_launch_t<double>(ctx, kt, a, max_group_rows);
    if (kt > K1W_MAX_KT) {
        using Fn = int (*)(pols_ctx *, int, const K1Args &, int64_t);
        static const Fn wide[2][4] = {{k1w_launch_f32_a, k1w_launch_f32_b, k1w_launch_f32_c, k1w_launch_f32_d},
                                      {k1w_launch_f64_a, k1w_launch_f64_b, k1w_launch_f64_c, k1w_launch_f64_d}};
        return wide[f32 ? 0 : 1][(kt - 16) / 4](ctx, kt, a, max_group_rows);
    }
    return f32 ? k1_launch_t<float>(ctx, kt, a, max_group_rows) : k1_launch_t<double>(ctx, kt, a, max_group_rows);
}
}  // namespace pols

// ------------------------------------------------------------------ POLS_TIMELINE=1 debugging aid
namespace pols {
int report_timeline(pols_ctx *ctx, const unsigned long long *d_dbg, int64_t n_groups, int n_stamps, const char *name) {
    std::vector<unsigned long long> h((size_t)n_groups * 8);
    POLS_HIP(hipStreamSynchronize(ctx->stream));
    POLS_HIP(hipMemcpy(h.data(), d_dbg, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::vector<double> phase(n_stamps, 0.0);
    double life = 0.0;
    // per-XCC span (s_memtime is per-XCD): concurrency = sum of lifetimes / span / CUs-per-XCC
    unsigned long long lo[8], hi[8];
    double sumlife[8] = {0};
    for (int x = 0; x < 8; ++x) { lo[x] = ~0ULL; hi[x] = 0; }
    for (int64_t g = 0; g < n_groups; ++g) {
        const unsigned long long *t = &h[(size_t)g * 8];
        for (int i = 0; i + 1 < n_stamps; ++i) phase[i] += (double)(t[i + 1] - t[i]);
        life += (double)(t[n_stamps - 1] - t[0]);
        const int x = (int)((t[6] >> 32) & 7);
        lo[x] = std::min(lo[x], t[0]);
        hi[x] = std::max(hi[x], t[n_stamps - 1]);
        sumlife[x] += (double)(t[n_stamps - 1] - t[0]);
    }
    std::fprintf(stderr, "[timeline] %s groups=%lld mean cycles/workgroup: life=%.0f |", name, (long long)n_groups, life / n_groups);
    for (int i = 0; i + 1 < n_stamps; ++i) std::fprintf(stderr, " p%d=%.0f", i, phase[i] / n_groups);
    double conc = 0.0, span = 0.0;
    int nx = 0;
    for (int x = 0; x < 8; ++x)
        if (hi[x] > lo[x]) { conc += sumlife[x] / (double)(hi[x] - lo[x]); span += (double)(hi[x] - lo[x]); ++nx; }
    std::fprintf(stderr, " | xccs=%d mean span=%.0f ticks, resident workgroups/CU=%.2f\n", nx, nx ? span / nx : 0.0,
                 ctx->num_cus ? conc / ctx->num_cus : 0.0);
    return POLS_OK;
}
}  // namespace pols
