// api_dynamic.hip -- the dynamic least-squares entries (rolling / expanding and recursive): the shared prologue (dyn_prep.hpp), the cached
// per-frame tables, a pure route picker per entry and one function per route (see "Dynamic routes" in DESIGN.md).  Host code only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "api_internal.hpp"
#include "dyn_prep.hpp"
#include "k3_rls.hpp"
#include "k4_rolling.hpp"

namespace pols {

// Dynamic models share the staging of a batch whose coefficient output has one row per input row, and the pre-processing the
// reference's Python layer / plugin bodies do around the solver (dyn_prep.hpp): validity from the null policy, sqrt(w) scaling, the
// ones column, nulls -> 0 -- on the device, behind the boundary.
struct DynState {
    int k = 0;                       // columns the kernels see: n_features + add_intercept
    bool post = false;               // predictions need the 1 / sqrt(w) un-scaling and / or the validity mask
    DynPrepArgs pa;
    pols_batch tables;               // the batch as build_chunk_tables should see it (validity bytes may now live on the device)
    bool deferred = false;           // the zero-filling rewrite of the columns has been left out (see dynamic_prologue's may_defer)
    std::vector<void *> outp;        // ... and these are the columns it would write
};

// may_defer: the caller has a kernel that masks invalid rows itself (the masked tile kernel of the rolling entry): the zero-filling rewrite
// of the columns -- a read and a write of the whole frame -- is skipped and left to dynamic_rewrite_deferred() should that kernel not be taken.
static int dynamic_prologue(pols_ctx *ctx, const pols_batch *b, int null_policy, pols_out *o, const int64_t **d_offs, int64_t *max_rows,
                            Staged *st, DynState *ds, bool may_defer = false) {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    if ((rc = check_batch(b, o, K4Y_KMAX))) return rc;
    if (null_policy < POLS_NULL_IGNORE || null_policy > POLS_NULL_DROP_WINDOW) return fail(POLS_ERR_INVALID, "unknown null_policy %d", null_policy);
    const int k = b->n_features + (b->add_intercept ? 1 : 0);
    ds->k = k;
    ds->tables = *b;
    std::memset(&ds->pa, 0, sizeof(ds->pa));
    if ((rc = upload_offsets(ctx, b->group_offsets, b->n_groups, d_offs, max_rows, b->offsets_generation))) return rc;
    if ((rc = stage_inputs(ctx, b, b->n_rows, k, o, st))) return rc;
    if (b->n_groups == 0 || b->n_rows == 0) return POLS_OK;
    const bool scan = st->valid == nullptr && !b->null_free;   // no validity bytes from the caller: a null is a NaN, the policy decides
    const bool has_w = st->w != nullptr, icpt = b->add_intercept != 0;
    bool some_invalid = !scan, some_null = false;
    const size_t colb = round256(dtype_size(b->dtype) * (size_t)b->n_rows);
    DynPrepArgs &pa = ds->pa;
    // (a caller's validity bytes without weights / intercept: the columns may still hold NaNs on the masked rows -- they are
    //  zero-filled like everywhere else, so that no prefix sum ever meets a NaN; null_free says there is nothing to fill)
    if (scan || has_w || icpt || (st->valid != nullptr && !b->null_free)) {
        // (the flag words lead on a 256-byte line of their own; sqrt(w) keeps its room without weights: the columns do not move)
        const size_t tabb = sizeof(void *) * (size_t)std::max(k, 1);
        void *xs = nullptr;
        Carve cv;
        cv.add(pa.flags, 256);
        cv.add(pa.valid_out, (size_t)b->n_rows);
        cv.add(pa.xtab, tabb);
        cv.add(pa.xout, tabb);
        cv.keep(pa.sw_out, colb, has_w);
        cv.add(pa.y_out, colb);
        cv.add(xs, colb * (size_t)k);
        if ((rc = carve(ctx, Work::DynPrep, cv))) return rc;
        std::vector<void *> outp((size_t)k);
        for (int j = 0; j < k; ++j) outp[(size_t)j] = column(xs, colb, (size_t)j);
        if ((rc = upload_small(ctx, const_cast<void **>(pa.xtab), st->x.data(), sizeof(void *) * (size_t)b->n_features))) return rc;
        if ((rc = upload_small(ctx, const_cast<void **>(pa.xout), outp.data(), sizeof(void *) * (size_t)k))) return rc;
        pa.y = st->y; pa.w = st->w;
        pa.k_user = b->n_features; pa.add_intercept = icpt ? 1 : 0; pa.null_policy = null_policy; pa.n_rows = b->n_rows;
        if (scan) {
            POLS_HIP(hipMemsetAsync(pa.flags, 0, 256, ctx->stream));
            if ((rc = dyn_scan_launch(ctx, b->dtype, pa))) return rc;
            int32_t flags[2] = {0, 0};
            POLS_HIP(hipMemcpyAsync(flags, pa.flags, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
            POLS_HIP(hipStreamSynchronize(ctx->stream));   // the host decides which path runs (mask-free tables are cached)
            some_invalid = flags[0] > 0;
            some_null = flags[1] > 0;
            if (some_invalid) {
                st->valid = pa.valid_out;
                ds->tables.valid = pa.valid_out;
                ds->tables.mem = POLS_MEM_DEVICE;
            }
        }
        if (has_w || icpt || some_invalid || some_null) {
            // (rows left out of the fit hold the nulls that put them there: zero-filled too, so that no kernel ever multiplies a NaN by 0)
            if (may_defer && !has_w && !icpt && st->valid != nullptr && !some_null) {    // (a null INSIDE a kept row has to be filled: no deferral)
                ds->deferred = true;                          // the columns stay the caller's; dynamic_rewrite_deferred() does this later if needed
                ds->outp.assign(outp.begin(), outp.end());
            } else {
                if ((rc = dyn_rewrite_launch(ctx, b->dtype, pa))) return rc;
                st->y = pa.y_out;
                st->x.assign(outp.begin(), outp.end());
            }
        }
    }
    ds->post = (has_w || st->valid != nullptr) && st->pred != nullptr;
    pa.pred = st->pred;
    pa.valid_post = st->valid;
    if (!has_w) pa.sw_out = nullptr;
    return POLS_OK;
}

static int dynamic_rewrite_deferred(pols_ctx *ctx, const pols_batch *b, Staged *st, DynState *ds) {
    if (!ds->deferred) return POLS_OK;
    int rc = dyn_rewrite_launch(ctx, b->dtype, ds->pa);
    if (rc) return rc;
    st->y = ds->pa.y_out;
    st->x.assign(ds->outp.begin(), ds->outp.end());
    ds->deferred = false;
    return POLS_OK;
}

// beyond 128 features a chunk carries a k x k state and a k x k total in HBM (16 MB at k = 1 024) and its workgroup an O(k^3)
// inversion: a few hundred long chunks instead of thousands of 64-row ones
static int64_t hbm_state_chunk(int64_t n_rows) { return std::max<int64_t>(64, (n_rows + 383) / 384); }

// Work::Tables of the dynamic entries: the RLS prior mean, then the column pointer table for more than 32 features
static int dynamic_tables(pols_ctx *ctx, const double *&mean0, const void *const *&xtab) {
    Carve cv;
    cv.add(mean0, sizeof(double) * K4Y_KMAX);
    cv.add(xtab, sizeof(void *) * K4Y_KMAX);
    return carve(ctx, Work::Tables, cv);
}
static int upload_column_table(pols_ctx *ctx, const Staged &st, int k, K4Args *a) {
    for (int j = 0; j < std::min(k, (int)POLS_MAX_FEATURES); ++j) a->x[j] = st.x[j];
    if (k <= POLS_MAX_FEATURES) return POLS_OK;
    const double *mean0 = nullptr;
    int rc = dynamic_tables(ctx, mean0, a->xtab);
    if (rc) return rc;
    return upload_small(ctx, const_cast<void **>(a->xtab), st.x.data(), sizeof(void *) * (size_t)k);
}

// Sequence-start bytes of the row-parallel dynamic kernels, cached per uploaded offsets.
static int ensure_start_flags(pols_ctx *ctx, const int64_t *d_offs, int64_t n_groups, int64_t n_rows, const uint8_t **flags) {
    auto &fc = ctx->start_flags;
    void *d = nullptr;
    int rc = grow(fc, round256((size_t)n_rows + 4), &d);
    if (rc) return rc;
    if (!fc.valid || fc.offs_id != ctx->offs_id || fc.n_groups != n_groups || fc.n_rows != n_rows) {
        fc.valid = false;
        if ((rc = k3c_start_flags(ctx, d_offs, n_groups, n_rows, static_cast<uint8_t *>(d)))) return rc;
        fc.valid = true; fc.offs_id = ctx->offs_id; fc.n_groups = n_groups; fc.n_rows = n_rows;
    }
    *flags = static_cast<const uint8_t *>(d);
    return POLS_OK;
}

// first rows of the packed tiles of a frame (whole sequences per tile, first fit in frame order; N appended) -- see ensure_packed_tiles
static void packed_tile_starts(const int64_t *offs, int64_t n_groups, int64_t N, int64_t tile_rows, std::vector<int64_t> *first) {
    first->clear();
    int64_t base = -1;
    for (int64_t g = 0; g < n_groups; ++g) {
        if (offs[g + 1] == offs[g]) continue;
        if (base < 0 || offs[g + 1] - base > tile_rows) { first->push_back(offs[g]); base = offs[g] & ~(int64_t)3; }
    }
    first->push_back(N);
}

// Packed tiles of the row-parallel dynamic kernels (K3c / K4c): no sequence longer than a tile (less the three rows a tile may start
// before its first sequence) -> tiles are cut at sequence starts, whole sequences, first fit in frame order; tile t owns rows
// [map[t], map[t + 1]).  Taken when the tiles come out at least 70 % full; *n_tiles = 0 otherwise.  Cached per frame (ctx->k3c).
static int ensure_packed_tiles(pols_ctx *ctx, const pols_batch *b, int64_t tile_rows, int64_t max_rows, const int64_t **map, int64_t *n_tiles) {
    *map = nullptr; *n_tiles = 0;
    if (max_rows > tile_rows - 3) return POLS_OK;
    const int64_t N = b->n_rows;
    auto &tc = ctx->k3c;
    void *dmap = nullptr;
    int rc = grow(tc, round256(sizeof(int64_t) * (size_t)(b->n_groups + 2)), &dmap);
    if (rc) return rc;
    if (!tc.valid || tc.offs_id != ctx->offs_id || tc.n_groups != b->n_groups || tc.n_rows != N || tc.tile_rows != tile_rows) {
        tc.valid = false;
        std::vector<int64_t> first;
        packed_tile_starts(b->group_offsets, b->n_groups, N, tile_rows, &first);
        const int64_t nt = (int64_t)first.size() - 1;
        tc.n_tiles = nt * tile_rows * 7 <= N * 10 ? nt : 0;
        if (tc.n_tiles && (rc = upload_small(ctx, dmap, first.data(), sizeof(int64_t) * first.size()))) return rc;
        tc.valid = true; tc.offs_id = ctx->offs_id; tc.n_groups = b->n_groups; tc.n_rows = N; tc.tile_rows = tile_rows;
    }
    *n_tiles = tc.n_tiles;
    if (tc.n_tiles) *map = static_cast<const int64_t *>(dmap);
    return POLS_OK;
}

// K3c's halo form: per tile of tile_rows rows the first row of the sequence that holds the row in front of the tile (tile 0: 0) -- the
// prior's decay up to the tile is then exact.  Cached per frame (ctx->k3h).
static int ensure_tile_seq0(pols_ctx *ctx, const pols_batch *b, int64_t tile_rows, int64_t n_tiles, const int64_t **map) {
    *map = nullptr;
    const int64_t N = b->n_rows;
    auto &tc = ctx->k3h;
    void *dmap = nullptr;
    int rc = grow(tc, round256(sizeof(int64_t) * (size_t)(n_tiles + 1)), &dmap);
    if (rc) return rc;
    if (!tc.valid || tc.offs_id != ctx->offs_id || tc.n_groups != b->n_groups || tc.n_rows != N || tc.tile_rows != tile_rows) {
        tc.valid = false;
        std::vector<int64_t> first((size_t)n_tiles, 0);
        const int64_t *offs = b->group_offsets;
        int64_t g = 0;
        for (int64_t t = 1; t < n_tiles; ++t) {
            const int64_t row = t * tile_rows - 1;
            while (g + 1 < b->n_groups && offs[g + 1] <= row) ++g;            // the (non-empty) group that holds `row`
            first[(size_t)t] = offs[g];
        }
        if ((rc = upload_small(ctx, dmap, first.data(), sizeof(int64_t) * first.size()))) return rc;
        tc.valid = true; tc.offs_id = ctx->offs_id; tc.n_groups = b->n_groups; tc.n_rows = N; tc.tile_rows = tile_rows;
    }
    *map = static_cast<const int64_t *>(dmap);
    return POLS_OK;
}

// ------------------------------------------------------------------ chunk tables
// Host-side tables shared by the chunk-parallel dynamic kernels (K4 rolling, K3s RLS scan): validity prefix
// (cnt / vidx), per-group warm-up constants of solve_rolling_ols (ls.rs:881-900) and the chunk list; uploaded to
// ctx->chunk_cache's table, the per-chunk totals live in Work::Gram (`slots` doubles per chunk).  Only the tables of a mask-free batch on
// the uploaded offsets are kept for the next call: other offsets (a compacted frame) can share every key the cache compares.
struct ChunkWalk {
    std::vector<K4Group> groups;
    std::vector<K4Chunk> chunks;
    std::vector<int32_t> order, cnt, vidx;   // cnt / vidx: only with host validity bytes
};

// The host walk: groups (with the warm-up constants from the host validity bytes `hv`, or the null-free ones), chunks of chunk_len rows
// and the work order of the wave-per-chunk kernels.
static int walk_chunks(const pols_batch *b, const uint8_t *hv, int64_t mp, int64_t chunk_len, ChunkWalk *w) {
    const int64_t N = b->n_rows;
    w->groups.resize((size_t)b->n_groups);
    if (hv) { w->cnt.resize((size_t)N); w->vidx.assign((size_t)N, -1); }
    for (int64_t g = 0; g < b->n_groups; ++g) {
        const int64_t s = b->group_offsets[g], e = b->group_offsets[g + 1], n = e - s;
        if (n > 0x7fffffffLL) return fail(POLS_ERR_UNSUPPORTED, "group longer than 2^31 rows");
        K4Group G;
        G.start = s; G.end = e; G.first_chunk = (int32_t)w->chunks.size();
        int64_t mpv = mp, n_valid = 0;                                                           // ls.rs:881-891
        bool reached = false;
        if (hv) {
            int32_t c = 0;
            for (int64_t i = 0; i < n; ++i) {
                if (hv[s + i]) { w->vidx[(size_t)(s + c)] = (int32_t)i; ++c; }
                w->cnt[(size_t)(s + i)] = c;
                if (!reached) {
                    n_valid = c;
                    if (c == mp) { mpv = i + 1; reached = true; }
                }
            }
        } else {
            n_valid = std::min(n, mp);
            if (n >= mp) { mpv = mp; reached = true; }
        }
        G.mpv = mpv;
        G.gate_n = n_valid;
        G.all_nan = (n < std::max(n_valid, mp)) ? 1 : 0;                                         // ls.rs:893-900
        w->groups[(size_t)g] = G;
        for (int64_t t = s, ci = 0; t < e; t += chunk_len, ++ci)
            w->chunks.push_back(K4Chunk{t, std::min(e, t + chunk_len), (int32_t)g, (int32_t)ci});
    }
    // work order of the wave-per-chunk kernels (K4Args::order): chunk ids sorted by length, longest first (stable: equal chunks keep their order) --
    // sequences of 5 .. 4 000 rows cut at ~500 gave waves whose four chunks were 30 and 480 rows long: RLS at 12 features 2.9 ms on a log-normal
    // frame against 0.9 ms on equal sequences (scripts/bench_dyn_spread.py)
    const std::vector<K4Chunk> &chunks = w->chunks;
    w->order.resize(chunks.size());
    for (size_t i = 0; i < w->order.size(); ++i) w->order[i] = (int32_t)i;
    if (chunks.size() < 0x7fffffffULL)
        std::stable_sort(w->order.begin(), w->order.end(), [&](int32_t x, int32_t y) { return chunks[(size_t)x].t1 - chunks[(size_t)x].t0 > chunks[(size_t)y].t1 - chunks[(size_t)y].t0; });
    return POLS_OK;
}

// Validity bytes that live on the device: cnt / vidx are built there and the uploaded groups -- which carry the null-free constants
// mpv = min_periods, gate_n = min(rows, min_periods) -- are patched from the bytes (all_nan only depends on the group's length: n_valid
// never exceeds min_periods).  The slab counts, slab bases and compacted offsets of the pass live behind the tables.
static int patch_tables_on_device(pols_ctx *ctx, const pols_batch *b, int64_t mp, const ChunkTables &t) {
    const int64_t N = b->n_rows, n_slabs = (N + 255) / 256;
    int rc;
    RowCompactArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    ra.valid = b->valid; ra.offs = static_cast<const int64_t *>(ctx->offsets.buf.ptr);
    ra.n_rows = N; ra.n_groups = b->n_groups; ra.n_slabs = n_slabs;
    ra.slab_cnt = t.slab_cnt; ra.slab_base = t.slab_base; ra.c_offs = t.c_offs;
    ra.slab_gfirst = nullptr;
    if ((rc = row_compact_offsets_launch(ctx, ra))) return rc;
    ValidTablesArgs va;
    std::memset(&va, 0, sizeof(va));
    va.valid = b->valid; va.offs = ra.offs; va.n_rows = N; va.n_groups = b->n_groups; va.n_slabs = n_slabs;
    va.slab_base = ra.slab_base; va.c_offs = ra.c_offs;
    va.cnt = t.cnt; va.vidx = t.vidx;
    va.groups = t.groups; va.min_periods = mp;
    return valid_tables_launch(ctx, va);
}

static int build_chunk_tables(pols_ctx *ctx, const pols_batch *b, int64_t mp, int slots, K4Args *a, int64_t min_chunk = 64, int64_t max_chunk = 512) {
    int rc;
    const int64_t N = b->n_rows;
    std::vector<uint8_t> hvalid;
    const uint8_t *hv = nullptr;
    // validity bytes that live on the device: the prefix tables are built there too (dyn_prep.hip valid_tables_launch) -- copying the
    // bytes home, walking every row and uploading two int32 tables was 40+ ms of a 10 M-row call whose kernels take 3-5
    const bool uploaded = ctx->offsets.valid && b->group_offsets == ctx->offs_host;
    const bool dev_tables = b->valid && b->mem == POLS_MEM_DEVICE && uploaded && b->n_groups > 0 && N > 0;
    if (b->valid && !dev_tables) {
        if (b->mem == POLS_MEM_DEVICE) {
            hvalid.resize((size_t)N);
            POLS_HIP(hipMemcpyAsync(hvalid.data(), b->valid, (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
            POLS_HIP(hipStreamSynchronize(ctx->stream));
            hv = hvalid.data();
        } else {
            hv = b->valid;
        }
    }
    // one lane (or wave / workgroup) per chunk: short chunks = more parallelism in the walk, longer chunk list for the scan
    // (measured on the 1M-row sequence: 64-row chunks = 15 625 lanes beat 32- and 16-row chunks -- the per-lane row loads are
    // uncoalesced and more concurrent lanes cost more in the memory system than they win in parallelism)
    const int64_t chunk_len = std::min<int64_t>(std::max(max_chunk, min_chunk), std::max<int64_t>(min_chunk, N / 16384));
    auto &cc = ctx->chunk_cache;
    const bool cacheable = !hv && !dev_tables && uploaded;
    ChunkTables t;
    Carve cv;
    void *tot = nullptr;
    auto hand_out = [&](int64_t n_chunks) {
        a->groups = reinterpret_cast<const K4Group *>(t.groups);
        a->chunks = reinterpret_cast<const K4Chunk *>(t.chunks);
        a->order = t.order; a->cnt = t.cnt; a->vidx = t.vidx;
        a->n_chunks = n_chunks; a->n_groups = (int32_t)b->n_groups;
        a->totals = static_cast<double *>(tot);
        a->chunk_len = (int32_t)chunk_len;
    };
    if (cacheable && cc.valid && cc.offs_id == ctx->offs_id && cc.n_groups == b->n_groups &&
        cc.n_rows == N && cc.mp == mp && cc.chunk_len == (int32_t)chunk_len) {      // same frame as the last call
        if ((rc = ensure_scratch(ctx, Work::Gram, sizeof(double) * (size_t)slots * std::max<size_t>(1, (size_t)cc.n_chunks), &tot))) return rc;
        chunk_tables_layout(cv, t, sizeof(K4Group), sizeof(K4Chunk), b->n_groups, cc.n_chunks, N, false, false);
        cv.place(cc.buf.ptr);
        hand_out(cc.n_chunks);
        return POLS_OK;
    }
    ChunkWalk w;
    if ((rc = walk_chunks(b, hv, mp, chunk_len, &w))) return rc;
    chunk_tables_layout(cv, t, sizeof(K4Group), sizeof(K4Chunk), b->n_groups, (int64_t)w.chunks.size(), N, hv || dev_tables, dev_tables);
    cc.valid = false;                                  // the table is about to be rewritten
    if ((rc = carve(cc, cv))) return rc;
    if ((rc = ensure_scratch(ctx, Work::Gram, sizeof(double) * (size_t)slots * std::max<size_t>(1, w.chunks.size()), &tot))) return rc;
    if ((rc = upload_small(ctx, t.groups, w.groups.data(), sizeof(K4Group) * w.groups.size()))) return rc;   // locals: through the pinned ring
    if ((rc = upload_small(ctx, t.chunks, w.chunks.data(), sizeof(K4Chunk) * w.chunks.size()))) return rc;
    if ((rc = upload_small(ctx, t.order, w.order.data(), sizeof(int32_t) * w.order.size()))) return rc;
    if (hv) {
        if ((rc = upload_small(ctx, t.cnt, w.cnt.data(), sizeof(int32_t) * (size_t)N))) return rc;
        if ((rc = upload_small(ctx, t.vidx, w.vidx.data(), sizeof(int32_t) * (size_t)N))) return rc;
    }
    if (dev_tables && (rc = patch_tables_on_device(ctx, b, mp, t))) return rc;
    hand_out((int64_t)w.chunks.size());
    if (cacheable) {
        cc.offs_id = ctx->offs_id; cc.n_groups = b->n_groups; cc.n_rows = N; cc.mp = mp; cc.n_chunks = a->n_chunks;
        cc.chunk_len = (int32_t)chunk_len; cc.valid = true;
    }
    return POLS_OK;
}

// ------------------------------------------------------------------ what the routes of both entries share
// One call of a dynamic entry: what every route needs.
struct DynCall {
    pols_ctx *ctx = nullptr;
    const pols_batch *b = nullptr;
    pols_out *o = nullptr;
    Staged st;
    DynState ds;
    const int64_t *d_offs = nullptr;     // device offsets
    int64_t max_rows = 0;                // rows of the longest sequence
    int k = 0;                           // features the kernels see (the intercept column included)
};

// The row-parallel kernels (K3c, K4c) make every access a 16-byte one down the row axis: 16-byte aligned columns / outputs, validity
// bytes (where there are any) on a 4-byte boundary.
static bool rowpar_aligned(const Staged &st, int k) {
    bool ok = aligned16(st.y) && (!st.coef || aligned16(st.coef)) && (!st.pred || aligned16(st.pred)) &&
              (!st.valid || (reinterpret_cast<uintptr_t>(st.valid) & 3) == 0);
    for (int j = 0; j < k && ok; ++j) ok = aligned16(st.x[j]);
    return ok;
}

// The epilogue of every route.  Post::Full: the post pass masks the predictions of the rows left out and un-scales by 1 / sqrt(w);
// Post::UnscaleOnly: the route's kernels wrote the null predictions themselves, the pass is only needed for the un-scaling.
enum class Post { Full, UnscaleOnly };
static int finish(DynCall &c, Post post) {
    int rc;
    if (c.ds.post && (post == Post::Full || c.ds.pa.sw_out) && (rc = dyn_post_launch(c.ctx, c.b->dtype, c.ds.pa))) return rc;
    return unstage_outputs(c.ctx, c.b, c.b->n_rows, c.k, c.o, c.st);
}

// Chunk sizes and totals slots of the lane / wave / workgroup-per-chunk kernels.  wave_p (K3p / K4p, k4p_wide.hip): a sequence of up to
// 1 024 rows is one chunk -- thousands of sequences are parallelism enough, only the few beyond 1 024 rows are cut then (n_groups >= 4096),
// and only they pay the totals pass and the scan.
struct ChunkPlan {
    int64_t pchunk, min_chunk, max_chunk;
    int slots;                           // doubles per chunk in the totals (`extra`: the RLS decay)
    bool wide;                           // more than 8 features: chunk-major totals for the wave / workgroup-per-chunk kernels
};
static ChunkPlan chunk_plan(int k, bool wave_p, int64_t longest, int64_t n_rows, int64_t n_groups, int extra) {
    ChunkPlan pl;
    pl.wide = k > K4_KMAX;
    pl.pchunk = (longest <= 1024 || n_groups >= 4096) ? 1024 : std::min<int64_t>(1024, std::max<int64_t>(256, n_rows / 16384));
    pl.min_chunk = wave_p ? pl.pchunk : (k > K4X_KMAX ? hbm_state_chunk(n_rows) : 64);
    pl.max_chunk = wave_p ? pl.pchunk : std::max<int64_t>(512, pl.min_chunk);
    pl.slots = (pl.wide ? k * k + k : k * (k + 1) / 2 + k) + extra;
    return pl;
}
// zeroed K4Args with the chunk tables of `tables` and the totals layout of the plan
static int chunked_args(pols_ctx *ctx, const pols_batch *tables, int64_t mp, const ChunkPlan &pl, K4Args *a) {
    std::memset(a, 0, sizeof(*a));
    int rc = build_chunk_tables(ctx, tables, mp, pl.slots, a, pl.min_chunk, pl.max_chunk);
    if (rc) return rc;
    if (pl.wide) { a->tot_cs = pl.slots; a->tot_qs = 1; }               // chunk-major
    else { a->tot_cs = 1; a->tot_qs = a->n_chunks; }                    // component-major for the lane-per-chunk kernels
    return POLS_OK;
}
// ... and what every chunk kernel reads from the call itself: the columns (a device table beyond 32 features), validity bytes, outputs
static int chunk_kernel_args(DynCall &c, int64_t mp, const ChunkPlan &pl, K4Args *a) {
    int rc = chunked_args(c.ctx, &c.ds.tables, mp, pl, a);
    if (rc) return rc;
    a->y = c.st.y; a->valid = c.st.valid;
    a->coef = c.st.coef; a->pred = c.st.pred; a->k = c.k;
    return upload_column_table(c.ctx, c.st, c.k, a);
}

// ------------------------------------------------------------------ recursive least squares
// Rows: the row-parallel, read-once kernel K3c (k3c_scan.hip) up to 10 features, whatever the sequence lengths; Scan: the chunk-parallel
// kernels (K3s lane-per-chunk / K3sw, K3p wave-per-chunk from 9 features / K3x, K3y workgroup-per-chunk from 33); Seq: K3, the
// wave-per-sequence P-form recursion, for short sequences.
enum class RlsRoute { Rows, Scan, Seq };
struct RlsFacts {
    int k;
    int64_t max_rows;
    bool aligned;                        // rowpar_aligned
    RlsEngine engine;
};
static RlsRoute pick_rls_route(const RlsFacts &f) {
    if (f.k <= K3C_KMAX && f.engine != RlsEngine::Seq && f.engine != RlsEngine::Chunk && f.aligned) return RlsRoute::Rows;
    const bool wide = f.k > K4_KMAX;
    bool scan = f.max_rows > 4096 || wide;                   // long sequences, or more features than K3 holds
    if (f.engine == RlsEngine::Seq && !wide) scan = false;
    if (f.engine == RlsEngine::Scan || f.engine == RlsEngine::Chunk) scan = true;
    return scan ? RlsRoute::Scan : RlsRoute::Seq;
}

struct RlsCall : DynCall {
    double ff = 1.0, p0 = 0.0;           // forgetting factor (ls.rs:513-517), initial_state_covariance
    const double *mean0 = nullptr;       // device, k values, or nullptr
};

static int rls_route_rows(RlsCall &c) {
    pols_ctx *ctx = c.ctx;
    const pols_batch *b = c.b;
    const Staged &st = c.st;
    const RlsEngine engine = ctx->opt.rls_engine;
    int rc;
    const int kf = c.k;
    const int64_t N = b->n_rows, tile_rows = k3c_tile_rows(kf), n_tiles = (N + tile_rows - 1) / tile_rows;
    const int64_t n_blocks = (n_tiles + 63) / 64;
    const size_t b_rec = sizeof(double) * K3C_NCP * (size_t)n_tiles, b_int = sizeof(int32_t) * (size_t)n_tiles,
                 b_brec = sizeof(double) * K3C_NCP * (size_t)n_blocks, b_bint = sizeof(int32_t) * (size_t)n_blocks;
    K3cArgs a;
    std::memset(&a, 0, sizeof(a));
    Carve cv;
    cv.add(a.rec, b_rec); cv.add(a.carry, b_rec);
    cv.add(a.rec_closed, b_int); cv.add(a.carry_open, b_int);
    cv.add(a.brec, b_brec); cv.add(a.bcarry, b_brec);
    cv.add(a.brec_closed, b_bint);
    if ((rc = carve(ctx, Work::K3cRecords, cv))) return rc;
    if ((rc = ensure_start_flags(ctx, c.d_offs, b->n_groups, N, &a.start))) return rc;
    // No sequence longer than a tile (less the three rows a tile may start before its first sequence): tiles are cut at sequence
    // starts -- whole sequences, first fit in frame order -- and need no carry-in, so ONE launch reads and writes the frame once.
    // Taken when the packed tiles are at least 70 % full (the two-pass form costs about 1.5 launches of full tiles).
    int64_t n_packed = 0;
    if (engine != RlsEngine::Scan && (rc = ensure_packed_tiles(ctx, b, tile_rows, c.max_rows, &a.tile_row0, &n_packed))) return rc;
    a.y = st.y; a.valid = st.valid;
    for (int j = 0; j < kf; ++j) a.x[j] = st.x[j];
    a.n_rows = N; a.coef = st.coef; a.pred = st.pred; a.mean0 = c.mean0;
    a.ff = c.ff; a.p0 = c.p0;
    a.n_tiles = n_packed ? n_packed : n_tiles; a.k = kf;
    a.all_closed = n_packed || c.max_rows <= tile_rows ? 1 : 0;   // (any tile_rows consecutive rows then hold a sequence start)
    // A finite half-life bounds how far back a row's state reaches: with ff^H <= 2^-36 for H = 256 .. 2 048 rows (half_life <= 56.9) a tile
    // re-accumulates its carry-in from the H rows in front of it -- one launch, no records, no scan over the tiles (k3c_scan.hip, step H).
    // Null-free frames only (a masked row does not decay the state, so the distance to the tile is not the row distance);
    // POLS_RLS_ENGINE=scan keeps the exact scan, which also serves half_life = None and the longer half-lives.
    const int32_t halo = n_packed || st.valid || engine == RlsEngine::Scan || kf > K3C_HALO_KMAX ? 0 : k3c_halo_batches(a.ff);
    if (halo) {
        if ((rc = ensure_tile_seq0(ctx, b, tile_rows, n_tiles, &a.tile_seq0))) return rc;
        a.halo_batches = halo; a.log2ff = std::log2(a.ff); a.ffstep = std::pow(a.ff, (double)(tile_rows - 4));
        a.fresh_need = (int32_t)std::min<double>(std::ceil(-32.0 / a.log2ff), 256.0 * halo - 4.0);
        // ... and when the rows that matter all lie in the ONE tile in front (H <= 1 024 = a four-wave tile, up to 6 features), that tile's own
        // aggregate is all the carry-in needs: the look-back-one form (k3c_scan.hip MODE 3) -- every tile publishes its aggregate early, picks up
        // its predecessor's behind its own scan, and re-reads nothing.  POLS_RLS_ENGINE=halo keeps the halo form.
        const size_t gbytes = (size_t)n_tiles * 32 * 16;
        if (kf <= 6 && halo <= 4 && tile_rows == 1024 && n_tiles > 1 && gbytes < ((size_t)1 << 31) && engine != RlsEngine::Halo) {
            void *g = nullptr;
            bool fresh = false;
            if ((rc = grow(ctx->k3c_gran, gbytes, &g, &fresh))) return rc;
            if (fresh) POLS_HIP(hipMemsetAsync(g, 0, ctx->k3c_gran.cap, ctx->stream));       // no stale tag may survive
            a.gran = g; a.gran_bytes = (int64_t)gbytes; a.epoch = ++ctx->k3c_epoch;
            a.spin_limit = ctx->opt.rls_spin_limit >= 0 ? ctx->opt.rls_spin_limit : 64;
            a.early_publish = ctx->opt.rls_early;
        }
    }
    if ((rc = k3c_launch(ctx, b->dtype, a))) return rc;
    return finish(c, Post::UnscaleOnly);     // (the kernel writes the null predictions of the rows left out itself)
}

static int rls_route_scan(RlsCall &c) {
    pols_ctx *ctx = c.ctx;
    const pols_batch *b = c.b;
    const int k = c.k;
    const bool wide = k > K4_KMAX, xwide = k > POLS_MAX_FEATURES;
    // 9..32 features: one wave per chunk with the covariance distributed over its registers (K3p, k4p_wide.hip).  A sequence of up to
    // 1 024 rows is one chunk (the recursion starts from the prior: no totals, no scan); POLS_RLS_ENGINE=chunk keeps k4w_wide.hip.
    const bool wave_p = wide && !xwide && ctx->opt.rls_engine != RlsEngine::Chunk;
    const ChunkPlan pl = chunk_plan(k, wave_p, c.max_rows, b->n_rows, b->n_groups, 1);
    K4Args a;
    int rc = chunk_kernel_args(c, 1, pl, &a);
    if (rc) return rc;
    a.ff = c.ff; a.p0 = c.p0; a.mean0 = c.mean0;
    if (wave_p) rc = k4p_launch(ctx, b->dtype, a, true, c.max_rows <= pl.pchunk);
    else rc = k > K4X_KMAX ? k3y_launch(ctx, b->dtype, a) : xwide ? k3x_launch(ctx, b->dtype, a) : (wide ? k3sw_launch(ctx, b->dtype, a) : k3s_launch(ctx, b->dtype, a));
    if (rc) return rc;
    return finish(c, Post::Full);
}

static int rls_route_seq(RlsCall &c) {
    K3Args a;
    std::memset(&a, 0, sizeof(a));
    a.y = c.st.y; a.valid = c.st.valid;
    for (int j = 0; j < std::min<int>(c.k, POLS_MAX_FEATURES); ++j) a.x[j] = c.st.x[j];
    a.offs = c.d_offs;
    a.n_groups = c.b->n_groups;
    a.coef = c.st.coef; a.pred = c.st.pred;
    a.k = c.k;
    a.forgetting_factor = c.ff;
    a.initial_state_covariance = c.p0;
    a.mean0 = c.mean0;
    int rc = k3_launch(c.ctx, c.b->dtype, a);
    if (rc) return rc;
    return finish(c, Post::Full);
}

// ------------------------------------------------------------------ rolling least squares
// Tiles: the row-parallel tile kernel K4c (k4c_rolling.hip) on a null-free frame; Compacted: the drop family on a frame with nulls --
// the valid rows compacted (or gathered) in front of K4c / K4p; Masked: the fixed window ("drop_window") on a frame with nulls -- K4c with
// invalid rows as zero rows behind a per-row solve table; Chunks: the chunk-parallel kernels K4 / K4w / K4p / K4x / K4y.
enum class RollingRoute { Tiles, Compacted, Masked, Chunks };
struct RollingFacts {
    int k;
    int64_t window, min_periods;         // min_periods resolved (ls.rs:860)
    bool drop;                           // the drop family: the window is the last `window` VALID rows (ls.rs:947-950)
    bool has_valid, valid_on_device;     // validity bytes exist (after the prologue) / the chunk tables would see them on the device
    bool aligned;                        // rowpar_aligned
    int64_t n_rows, max_rows;
    bool packed;                         // packed tiles were taken (ensure_packed_tiles): whole sequences per tile, any window
    RollingEngine engine;
};
// K4c on the compacted valid rows needs the window inside the halo forms or sequences that pack (fewer valid rows than rows)
static bool compacted_fits_tiles(const RollingFacts &f) {
    return f.k <= K4C_KMAX && (f.window <= k4c_max_window(f.k) || f.max_rows <= K4C_PACKED_ROWS - 3);
}
// What the tile kernel needs before the window is looked at -- null-free frames: with every row valid the "drop" deque and the fixed
// window are the same sums; masked frames: "drop_window" with validity bytes on the device.
static bool tiles_possible(const RollingFacts &f) {
    return f.k <= K4C_KMAX && !f.has_valid && f.min_periods <= f.window && f.engine != RollingEngine::Chunk && f.aligned;
}
static bool masked_possible(const RollingFacts &f) {
    return !f.drop && f.has_valid && f.valid_on_device && f.k <= K4C_KMAX && f.min_periods <= f.window && f.engine != RollingEngine::Chunk &&
           f.engine != RollingEngine::NoCompact && f.n_rows >= 8 && f.aligned;
}
// the entry asks for packed tiles (an upload, cached per frame) only where a tile route may take them
static bool wants_packed_tiles(const RollingFacts &f) { return (tiles_possible(f) || masked_possible(f)) && f.engine != RollingEngine::Halo; }

// The FIRST route to try; Compacted and Masked can still decline (see the routes).
static RollingRoute pick_rolling_route(const RollingFacts &f) {
    // whole sequences per tile when none is longer than one: no window reaches outside its tile, no halo, any window;
    // otherwise the halo waves cover windows up to 508 rows (252 from 7 features on)
    const bool window_fits = f.packed || f.window <= k4c_max_window(f.k);
    if (tiles_possible(f) && window_fits) return RollingRoute::Tiles;
    // (11..32 features, and up to 10 where the window / packing conditions fail: the same compaction in front of the wave-per-chunk kernel K4p)
    const bool wave_ok = f.k > K4_KMAX && f.k <= POLS_MAX_FEATURES;
    if (f.drop && f.has_valid && f.min_periods <= f.window && (compacted_fits_tiles(f) || wave_ok) && f.engine != RollingEngine::Chunk &&
        f.engine != RollingEngine::NoCompact && f.n_rows >= 8)
        return RollingRoute::Compacted;
    if (masked_possible(f) && window_fits) return RollingRoute::Masked;
    return RollingRoute::Chunks;
}

struct RollingCall : DynCall {
    const pols_rolling_params *p = nullptr;
    int64_t window = 0, min_periods = 0; // min_periods resolved (ls.rs:860)
    bool drop = false;
    double alpha = 0.0;                  // clamped at 0 (ls.rs:865, 924-926)
    const int64_t *packed_map = nullptr; // packed tiles of the frame, where wants_packed_tiles() asked for them
    int64_t n_packed = 0;
};

// K4cArgs with the fields every tile launch sets.  packed: no window reaches outside a tile, so a window longer than a tile never
// fills -- any such is the same, and it is clamped to two tiles.  min_periods follows the clamp: on packed tiles no sequence has more
// than 1 021 rows, so a min_periods beyond the clamped window (2 048 < min_periods <= window_size) is "never enough rows" either way --
// all NaN, what the reference returns for a sequence shorter than min_periods (ls.rs:893-900) -- and the launch check
// (min_periods <= window) must not reject it.
static void k4c_set_window(const RollingCall &c, bool packed, K4cArgs *a) {
    a->window = packed ? std::min<int64_t>(c.window, 2 * K4C_PACKED_ROWS) : c.window;
    a->min_periods = std::min<int64_t>(c.min_periods, a->window);
}
static K4cArgs k4c_args(const RollingCall &c, const void *y, const void *const *x, int64_t n_rows, void *coef, void *pred, bool packed) {
    K4cArgs a;
    std::memset(&a, 0, sizeof(a));
    a.y = y;
    for (int j = 0; j < c.k; ++j) a.x[j] = x[j];
    a.n_rows = n_rows; a.coef = coef; a.pred = pred;
    a.alpha = c.alpha; a.k = c.k;
    k4c_set_window(c, packed, &a);
    return a;
}

static int rolling_route_tiles(RollingCall &c) {
    K4cArgs a = k4c_args(c, c.st.y, c.st.x.data(), c.b->n_rows, c.st.coef, c.st.pred, c.packed_map != nullptr);
    int rc = ensure_start_flags(c.ctx, c.d_offs, c.b->n_groups, c.b->n_rows, &a.start);
    if (rc) return rc;
    a.tile_row0 = c.packed_map; a.n_packed = c.n_packed;
    if ((rc = k4c_launch(c.ctx, c.b->dtype, a))) return rc;
    return finish(c, Post::Full);
}

// The chunk family.  9..32 features on a null-free frame, min_periods <= window: one wave per chunk, the inverse distributed over its
// registers and the sums kept beside it (K4p, k4p_wide.hip).  A sequence of up to 1 024 rows is one chunk; a chunk of a longer one re-sums
// the rows of the window in front of it, so cut sequences need a window of at most 1 024 rows or the scanned totals.
// POLS_ROLLING_ENGINE=chunk keeps k4w_wide.hip.  The FIXED window over rows ("drop_window") on frames with validity bytes on the device: the
// same kernel with the rows masked and the solves gated (the validity prefix is built on the device, dyn_prep.hip).
static int rolling_route_chunks(RollingCall &c) {
    pols_ctx *ctx = c.ctx;
    const pols_batch *b = c.b;
    const int k = c.k;
    const bool wide = k > K4_KMAX, xwide = k > POLS_MAX_FEATURES;                               // k4w_wide.hip / k4x_inverse.hip
    const bool wave_p = wide && !xwide && c.min_periods <= c.window && ctx->opt.rolling_engine != RollingEngine::Chunk &&
                        (c.st.valid == nullptr || (!c.drop && c.ds.tables.valid != nullptr && c.ds.tables.mem == POLS_MEM_DEVICE));
    const ChunkPlan pl = chunk_plan(k, wave_p, c.max_rows, b->n_rows, b->n_groups, 0);
    K4Args a;
    int rc = chunk_kernel_args(c, c.min_periods, pl, &a);
    if (rc) return rc;
    a.window = c.window; a.alpha = c.alpha; a.drop_mode = c.drop ? 1 : 0;
    if (wave_p) {
        a.use_totals = (c.max_rows > pl.pchunk && c.window > 1024) ? 1 : 0;    // cut sequences, a window too long to re-sum at every chunk start
        a.groups_end_row = b->n_rows;
        rc = k4p_launch(ctx, b->dtype, a, false, c.max_rows <= pl.pchunk);
    }
    else rc = k > K4X_KMAX ? k4y_launch(ctx, b->dtype, a) : xwide ? k4x_launch(ctx, b->dtype, a) : (wide ? k4w_launch(ctx, b->dtype, a) : k4_launch(ctx, b->dtype, a));
    if (rc) return rc;
    return finish(c, Post::Full);
}

// The compacted frame through K4p: chunk tables of the COMPACTED offsets (build_chunk_tables does not cache them), coefficients of the
// compacted rows into coef_c; the caller expands them.
static int compacted_wave_launch(RollingCall &c, const std::vector<int64_t> &c_offs, int64_t max_c, void *const *cols_c, void *coef_c) {
    const int64_t Nc = c_offs.back();
    pols_batch cb = *c.b;
    cb.group_offsets = c_offs.data(); cb.n_rows = Nc; cb.valid = nullptr;
    const ChunkPlan pl = chunk_plan(c.k, true, max_c, Nc, 0, 0);
    K4Args a;
    int rc = chunked_args(c.ctx, &cb, c.min_periods, pl, &a);
    if (rc) return rc;
    a.y = cols_c[0];
    for (int j = 0; j < c.k; ++j) a.x[j] = cols_c[j + 1];
    a.coef = coef_c; a.pred = nullptr;
    a.window = c.window; a.alpha = c.alpha; a.k = c.k; a.drop_mode = 1;
    a.use_totals = (max_c > pl.pchunk && c.window > 1024) ? 1 : 0;
    a.groups_end_row = Nc;
    return k4p_launch(c.ctx, c.b->dtype, a, false, max_c <= pl.pchunk);
}

// The drop family on a frame WITH nulls (the reference's default policy for rolling_ols, ls.rs:947-986): its deque of valid rows is
// the null-free window over the VALID rows, and a row left out repeats the last coefficients -- so the valid rows are compacted
// (dyn_prep.hip: slab counts, scan, scatter), the tile kernel (or K4p) runs on them, and an expansion pass forward-fills the coefficients
// onto the original rows and predicts them.  Up to 10 features the tile kernel GATHERS the valid rows through a source map and writes the
// frame's rows itself (k4c_kernel.inl GATHER, dyn_out_gather.inl): no compacted copy of the columns, no expansion pass;
// POLS_ROLLING_ENGINE=scatter keeps the three-pass form (and K4p still runs on compacted columns).
// Declines -- after the host has read the compacted offsets -- when a non-empty group holds fewer valid rows than min_periods (the
// reference then solves a window it never filled, :881-900: the chunk kernels reproduce that) or fewer than 8 rows are kept.
static int rolling_route_compacted(RollingCall &c, const RollingFacts &f, bool *declined) {
    pols_ctx *ctx = c.ctx;
    const pols_batch *b = c.b;
    const Staged &st = c.st;
    const int k = c.k;
    int rc;
    *declined = false;
    const int64_t N = b->n_rows, G = b->n_groups, n_slabs = (N + 255) / 256;
    const size_t sz = dtype_size(b->dtype), colb = round256(sz * (size_t)N);
    const bool on_tiles = compacted_fits_tiles(f);
    const bool gather = on_tiles && N < ((int64_t)1 << 31) && ctx->opt.rolling_engine != RollingEngine::Scatter;
    RowCompactArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    char *cols = nullptr;                              // k + 1 compacted columns: none when the tile kernel gathers
    Carve cv;
    cv.add(ra.slab_cnt, sizeof(uint32_t) * (size_t)n_slabs);
    cv.add(ra.slab_base, sizeof(int64_t) * (size_t)(n_slabs + 1));
    cv.add(ra.c_offs, sizeof(int64_t) * (size_t)(G + 1));
    cv.add(ra.slab_gfirst, sizeof(int64_t) * (size_t)n_slabs);
    cv.add(ra.in, sizeof(void *) * (size_t)(k + 1));
    cv.add(ra.out, sizeof(void *) * (size_t)(k + 1));
    cv.add(cols, gather ? 0 : colb * (size_t)(k + 1));
    if ((rc = carve(ctx, Work::RowCompact, cv))) return rc;
    std::vector<const void *> inp((size_t)k + 1);
    std::vector<void *> outp((size_t)k + 1);
    inp[0] = st.y;
    for (int j = 0; j < k; ++j) inp[(size_t)j + 1] = st.x[(size_t)j];
    for (int j = 0; j <= k; ++j) outp[(size_t)j] = gather ? nullptr : column(cols, colb, (size_t)j);
    if ((rc = upload_small(ctx, const_cast<void **>(ra.in), inp.data(), sizeof(void *) * (size_t)(k + 1)))) return rc;
    if ((rc = upload_small(ctx, const_cast<void **>(ra.out), outp.data(), sizeof(void *) * (size_t)(k + 1)))) return rc;
    ra.valid = st.valid;
    if ((rc = ensure_start_flags(ctx, c.d_offs, G, N, &ra.start))) return rc;
    ra.offs = c.d_offs; ra.n_rows = N; ra.n_groups = G; ra.n_slabs = n_slabs;
    ra.n_cols = k + 1; ra.k = k;
    if ((rc = row_compact_offsets_launch(ctx, ra))) return rc;
    std::vector<int64_t> c_offs((size_t)G + 1);
    POLS_HIP(hipMemcpyAsync(c_offs.data(), ra.c_offs, sizeof(int64_t) * (size_t)(G + 1), hipMemcpyDeviceToHost, ctx->stream));
    POLS_HIP(hipStreamSynchronize(ctx->stream));       // the host cuts the compacted frame into tiles and checks the warm-up quirk
    const int64_t Nc = c_offs[(size_t)G];
    int64_t max_c = 0;
    for (int64_t g = 0; g < G; ++g) {
        const int64_t nc = c_offs[(size_t)g + 1] - c_offs[(size_t)g];
        if (b->group_offsets[g + 1] > b->group_offsets[g] && nc < c.min_periods) { *declined = true; return POLS_OK; }
        max_c = std::max(max_c, nc);
    }
    if (Nc < 8) { *declined = true; return POLS_OK; }
    void *coef_c = nullptr;                            // coefficients of the compacted rows (the three-pass form)
    if (gather) {
        void *dsrc = nullptr;
        if ((rc = ensure_scratch(ctx, Work::GatherMap, round256(sizeof(int32_t) * (size_t)(Nc + 4)), &dsrc))) return rc;
        ra.src = static_cast<int32_t *>(dsrc);
        if ((rc = row_compact_srcmap_launch(ctx, ra))) return rc;
    } else {
        if ((rc = row_compact_scatter_launch(ctx, b->dtype, ra))) return rc;
        if ((rc = ensure_scratch(ctx, Work::CompactCoef, round256(sz * (size_t)Nc * (size_t)k), &coef_c))) return rc;
    }
    if (!on_tiles) {
        if ((rc = compacted_wave_launch(c, c_offs, max_c, outp.data(), coef_c))) return rc;
    } else {
        void *df = nullptr;
        if ((rc = ensure_scratch(ctx, Work::CompactStarts, round256((size_t)Nc + 4), &df))) return rc;
        if ((rc = k3c_start_flags(ctx, ra.c_offs, G, Nc, static_cast<uint8_t *>(df)))) return rc;
        K4cArgs a = gather ? k4c_args(c, st.y, st.x.data(), Nc, st.coef, st.pred, false) : k4c_args(c, outp[0], outp.data() + 1, Nc, coef_c, nullptr, false);
        a.start = static_cast<const uint8_t *>(df);
        if (gather) { a.src = ra.src; a.n_frame = N; a.fvalid = st.valid; a.fstart = ra.start; }
        if (max_c <= K4C_PACKED_ROWS - 3 && (ctx->opt.rolling_engine != RollingEngine::Halo || c.window > k4c_max_window(k))) {
            std::vector<int64_t> first;
            packed_tile_starts(c_offs.data(), G, Nc, K4C_PACKED_ROWS, &first);
            const int64_t nt = (int64_t)first.size() - 1;
            if (nt * K4C_PACKED_ROWS * 7 <= Nc * 10 || c.window > k4c_max_window(k)) {    // (a window beyond the halo forms: packed whatever the fill)
                void *dm = nullptr;
                k4c_set_window(c, true, &a);
                if ((rc = ensure_scratch(ctx, Work::CompactTiles, round256(sizeof(int64_t) * first.size()), &dm))) return rc;
                if ((rc = upload_small(ctx, dm, first.data(), sizeof(int64_t) * first.size()))) return rc;
                a.tile_row0 = static_cast<const int64_t *>(dm); a.n_packed = nt;
            }
        }
        if ((rc = k4c_launch(ctx, b->dtype, a))) return rc;
        if (gather) return finish(c, Post::UnscaleOnly);   // (the kernel wrote NaN predictions on the rows left out)
    }
    ra.coef_c = coef_c; ra.coef = st.coef; ra.pred = st.pred;
    if ((rc = row_compact_expand_launch(ctx, b->dtype, ra))) return rc;
    ctx->last_kernel += "_compacted";
    return finish(c, Post::Full);
}

// The FIXED window over rows ("drop_window", the RollingKwargs default, ls.rs:987-1029) on a frame WITH nulls, up to 10 features: the
// tile kernel with every invalid row a zero row (k4c_kernel.inl, MASKED) -- all rows solved from S_i = E(i) - E(i - window) -- behind a
// per-row table of which rows the reference solves (dyn_prep.hip: NaN before the warm-up row, the last solved row's coefficients where the
// n_valid_window gate is closed), applied by a fill pass.  Declines in one case: a sequence in which a valid row is older than the window
// when its warm-up ends is never subtracted by the reference (:989) -- the device flags it, the host reads the flag.
static int rolling_route_masked(RollingCall &c, bool *declined) {
    pols_ctx *ctx = c.ctx;
    const pols_batch *b = c.b;
    const Staged &st = c.st;
    const int k = c.k;
    int rc;
    *declined = false;
    const int64_t N = b->n_rows, G = b->n_groups, n_slabs = (N + 255) / 256, n_blk = (n_slabs + 1023) / 1024;
    const size_t b_blk = sizeof(unsigned long long) * (size_t)n_blk, b_r2 = sizeof(uint16_t) * (size_t)N,
                 b_s8 = sizeof(int64_t) * (size_t)(n_slabs + 1), b_g8 = sizeof(int64_t) * (size_t)(G + 1);
    RollMaskArgs ma;
    std::memset(&ma, 0, sizeof(ma));
    Carve cv;
    cv.add(ma.flag, 256);                              // the flag word on a line of its own
    cv.add(ma.blk_cnt, 2 * b_blk);                     // ... and blk_last, its second half
    cv.add(ma.incl, b_r2);
    cv.add(ma.code, b_r2);
    cv.add(ma.solved, (size_t)N + 4);
    cv.add(ma.slab_cnt, sizeof(uint32_t) * (size_t)n_slabs);
    cv.add(ma.slab_base, b_s8);
    cv.add(ma.slab_last, b_s8);
    cv.add(ma.slab_carry, b_s8);
    cv.add(ma.c_offs, b_g8);
    cv.add(ma.g_mpv, b_g8);
    cv.add(ma.g_gate, sizeof(int32_t) * (size_t)G);
    if ((rc = carve(ctx, Work::RowCompact, cv))) return rc;   // (Work::RowCompact: the compaction's, never live here)
    ma.blk_last = column(ma.blk_cnt, b_blk, 1);
    ma.valid = st.valid; ma.offs = c.d_offs; ma.n_rows = N; ma.n_groups = G; ma.n_slabs = n_slabs;
    ma.window = c.window; ma.min_periods = c.min_periods;
    if ((rc = roll_mask_tables_launch(ctx, ma))) return rc;
    int32_t flag = 0;
    POLS_HIP(hipMemcpyAsync(&flag, ma.flag, sizeof(flag), hipMemcpyDeviceToHost, ctx->stream));
    POLS_HIP(hipStreamSynchronize(ctx->stream));       // the host decides which kernel runs
    if (flag != 0) { *declined = true; return POLS_OK; }
    if ((rc = roll_mask_rows_launch(ctx, ma))) return rc;
    K4cArgs a = k4c_args(c, st.y, st.x.data(), N, st.coef, st.pred, c.packed_map != nullptr);
    if ((rc = ensure_start_flags(ctx, c.d_offs, G, N, &a.start))) return rc;
    a.valid = st.valid; a.solved = ma.solved;
    a.tile_row0 = c.packed_map; a.n_packed = c.n_packed;
    if ((rc = k4c_launch(ctx, b->dtype, a))) return rc;
    for (int j = 0; j < k; ++j) ma.x[j] = st.x[j];
    ma.coef = st.coef; ma.pred = st.pred; ma.k = k;
    if ((rc = roll_mask_fill_launch(ctx, b->dtype, ma))) return rc;
    return finish(c, Post::UnscaleOnly);     // (the kernel and the fill pass null the predictions of masked rows themselves)
}

}  // namespace pols

using namespace pols;

extern "C" {

// ------------------------------------------------------------------ defaults (ls.py:137-140, 156-160)
void pols_rls_params_default(pols_rls_params *p) {
    std::memset(p, 0, sizeof(*p));
    p->has_half_life = 0;
    p->initial_state_covariance = 10.0;
    p->initial_state_mean = nullptr;
    p->null_policy = POLS_NULL_DROP;
}

void pols_rolling_params_default(pols_rolling_params *p) {
    std::memset(p, 0, sizeof(*p));
    p->window_size = 1000000;
    p->min_periods = -1;
    p->use_woodbury = -1;
    p->alpha = 0.0;
    p->null_policy = POLS_NULL_DROP_WINDOW;
}

int pols_recursive_least_squares(pols_ctx *ctx, const pols_batch *b, const pols_rls_params *p, pols_out *o) {
    if (!p) return fail(POLS_ERR_INVALID, "params is NULL");
    RlsCall c;
    c.ctx = ctx; c.b = b; c.o = o;
    // (may_defer: the row-parallel kernel K3c masks invalid rows itself -- their values are SELECTED to zero, their decay is 1 -- so the zero-filling
    //  rewrite of the frame, a read and a write of every column, is left out on frames it takes: 10 000 x 1 000 x 6 with 3 % nulls 0.49 -> 0.31 ms)
    int rc = dynamic_prologue(ctx, b, p->null_policy, o, &c.d_offs, &c.max_rows, &c.st, &c.ds, true);
    if (rc) return rc;
    if (b->n_groups == 0 || b->n_rows == 0) return POLS_OK;
    if (o->resid) return fail(POLS_ERR_INVALID, "rls: residuals are target - predictions in the caller (least_squares.py:239)");
    c.k = c.ds.k;
    RlsFacts f{c.k, c.max_rows, rowpar_aligned(c.st, c.k), ctx->opt.rls_engine};
    RlsRoute route = pick_rls_route(f);
    if (route != RlsRoute::Rows && c.ds.deferred) {       // every other kernel wants zero-filled columns (and the rewritten ones are aligned)
        if ((rc = dynamic_rewrite_deferred(ctx, b, &c.st, &c.ds))) return rc;
        f.aligned = rowpar_aligned(c.st, c.k);
        route = pick_rls_route(f);
    }
    c.ff = p->has_half_life ? std::exp(std::log(0.5) / p->half_life) : 1.0;   // ls.rs:513-517
    c.p0 = p->initial_state_covariance;
    if (p->initial_state_mean) {
        const void *const *xtab = nullptr;
        if ((rc = dynamic_tables(ctx, c.mean0, xtab))) return rc;
        if ((rc = upload_small(ctx, const_cast<double *>(c.mean0), p->initial_state_mean, sizeof(double) * c.k))) return rc;   // the host array belongs to the caller (k values)
    }
    switch (route) {
    case RlsRoute::Rows: return rls_route_rows(c);
    case RlsRoute::Scan: return rls_route_scan(c);
    case RlsRoute::Seq: break;
    }
    return rls_route_seq(c);
}

int pols_rolling_least_squares(pols_ctx *ctx, const pols_batch *b, const pols_rolling_params *p, pols_out *o) {
    if (!p) return fail(POLS_ERR_INVALID, "params is NULL");
    RollingCall c;
    c.ctx = ctx; c.b = b; c.o = o; c.p = p;
    const RollingEngine engine = ctx->opt.rolling_engine;
    // ("drop_window" without weights / intercept on up to 10 features: the masked tile kernel reads the caller's columns as they are)
    // ("drop": the compaction in front of the tile kernel copies the VALID rows, which hold no null under that policy, out of the caller's columns)
    const bool may_defer = (p->null_policy == POLS_NULL_DROP_WINDOW || p->null_policy == POLS_NULL_DROP) && b->n_features <= K4C_KMAX &&
                           engine != RollingEngine::Chunk && engine != RollingEngine::NoCompact;
    int rc = dynamic_prologue(ctx, b, p->null_policy, o, &c.d_offs, &c.max_rows, &c.st, &c.ds, may_defer);
    if (rc) return rc;
    if (b->n_groups == 0 || b->n_rows == 0) return POLS_OK;
    if (o->resid) return fail(POLS_ERR_INVALID, "rolling: residuals are target - predictions in the caller (least_squares.py:239)");
    c.k = c.ds.k;
    if (p->window_size < 1) return fail(POLS_ERR_INVALID, "window_size must be >= 1");
    c.window = p->window_size;
    c.min_periods = p->min_periods >= 0 ? p->min_periods : std::min<int64_t>(c.k, c.window);    // ls.rs:860
    if (c.min_periods < 1) return fail(POLS_ERR_INVALID, "min_periods must be >= 1 (the reference indexes row min_periods - 1, ls.rs:941-943)");
    c.drop = p->null_policy == POLS_NULL_DROP || p->null_policy == POLS_NULL_DROP_ZERO || p->null_policy == POLS_NULL_DROP_Y_ZERO_X;   // ls.rs:947-950
    c.alpha = p->alpha > 0.0 ? p->alpha : 0.0;
    RollingFacts f{c.k, c.window, c.min_periods, c.drop, c.st.valid != nullptr, c.ds.tables.valid != nullptr && c.ds.tables.mem == POLS_MEM_DEVICE,
                   rowpar_aligned(c.st, c.k), b->n_rows, c.max_rows, false, engine};
    if (wants_packed_tiles(f) && (rc = ensure_packed_tiles(ctx, b, K4C_PACKED_ROWS, c.max_rows, &c.packed_map, &c.n_packed))) return rc;
    f.packed = c.packed_map != nullptr;
    bool declined = false;
    switch (pick_rolling_route(f)) {
    case RollingRoute::Tiles: return rolling_route_tiles(c);
    case RollingRoute::Compacted:
        if ((rc = rolling_route_compacted(c, f, &declined)) || !declined) return rc;
        break;
    case RollingRoute::Masked:
        if ((rc = rolling_route_masked(c, &declined)) || !declined) return rc;
        break;
    case RollingRoute::Chunks: break;
    }
    // no tile route took the frame: the chunk kernels want zero-filled columns
    if ((rc = dynamic_rewrite_deferred(ctx, b, &c.st, &c.ds))) return rc;
    return rolling_route_chunks(c);
}

}  // extern "C"
