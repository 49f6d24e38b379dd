// carve_check.cpp -- csrc/scratch_carve.hpp, csrc/table_layout.hpp, csrc/k17_split.hpp and csrc/fit_lds.hpp on the CPU (no HIP): test_scratch_carve_cpu.py compiles this with
// -fsanitize=address,undefined, runs it and compares every printed line with formulas written out by hand.  Each scenario carves a heap
// buffer of exactly total() bytes and writes every region end to end, so a region that reaches past the total is a sanitizer report.
// Output: "<scenario> <offset of every slot, -1 for nullptr> ... <total>"; "split <n_res> <max_res> <max_glb> : <list>".  The two cached
// tables print the slots of the build view, then those of the view a cache hit takes over the same buffer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fit_lds.hpp"
#include "k17_split.hpp"
#include "scratch_carve.hpp"
#include "table_layout.hpp"

using pols::Carve;

static char *g_base = nullptr;
static long off(const void *p) { return p ? (long)(static_cast<const char *>(p) - g_base) : -1; }
static void place(const Carve &cv) {
    std::free(g_base);
    g_base = static_cast<char *>(std::aligned_alloc(256, cv.total() ? cv.total() : 256));
    cv.place(g_base);
}
template <typename T> static void fill(T *p, size_t bytes) {
    if (p) std::memset(p, 0x5a, bytes);
}

// K12's Gram buffer: counts, parts and -- only when the frame is split -- the reduced matrices, which else ARE the parts
static void enet_gram(const char *name, size_t items, size_t G, size_t per, bool split) {
    int64_t *count = nullptr;
    double *part = nullptr, *gram = nullptr;
    Carve cv;
    cv.add(count, 8 * items);
    cv.add(part, 8 * items * per);
    cv.add(gram, split ? 8 * G * per : 0, &part);
    place(cv);
    fill(count, 8 * items); fill(part, 8 * items * per);
    if (split) fill(gram, 8 * G * per);
    std::printf("%s %ld %ld %ld %zu\n", name, off(count), off(part), off(gram), cv.total());
}

// a region that keeps its room: the staged outputs of a host batch (coef, pred, resid, status), `wanted` one bit each
static void kept(const char *name, unsigned wanted) {
    char *coef = nullptr, *pred = nullptr, *resid = nullptr;
    int32_t *status = nullptr;
    const size_t cb = 4 * 5 * 7, rb = 4 * 415, sb = 4 * 5;
    Carve cv;
    cv.keep(coef, cb, wanted & 1); cv.keep(pred, rb, wanted & 2); cv.keep(resid, rb, wanted & 4); cv.keep(status, sb, wanted & 8);
    place(cv);
    fill(coef, cb); fill(pred, rb); fill(resid, rb); fill(status, sb);
    std::printf("%s %ld %ld %ld %ld %zu\n", name, off(coef), off(pred), off(resid), off(status), cv.total());
}

// build_chunk_tables' table: the build carves it, a later view (the cache hit) places the same list over the kept buffer
static void chunk_tables(const char *name, int64_t G, int64_t chunks, int64_t N, bool prefix, bool on_device) {
    pols::ChunkTables t, hit;
    Carve cv, again;
    pols::chunk_tables_layout(cv, t, 40, 24, G, chunks, N, prefix, on_device);
    place(cv);
    const int64_t slabs = (N + 255) / 256;
    fill(t.groups, 40 * G); fill(t.chunks, 24 * chunks); fill(t.order, 4 * chunks); fill(t.cnt, 4 * N); fill(t.vidx, 4 * N);
    fill(t.slab_cnt, 4 * slabs); fill(t.slab_base, 8 * (slabs + 1)); fill(t.c_offs, 8 * (G + 1));
    pols::chunk_tables_layout(again, hit, 40, 24, G, chunks, N, prefix, on_device);
    again.place(g_base);
    std::printf("%s %ld %ld %ld %ld %ld %ld %ld %ld %zu", name, off(t.groups), off(t.chunks), off(t.order), off(t.cnt), off(t.vidx), off(t.slab_cnt),
                off(t.slab_base), off(t.c_offs), cv.total());
    std::printf(" %ld %ld %ld %ld %ld %ld %ld %ld %zu\n", off(hit.groups), off(hit.chunks), off(hit.order), off(hit.cnt), off(hit.vidx),
                off(hit.slab_cnt), off(hit.slab_base), off(hit.c_offs), again.total());
}

// ensure_segments' tables, the same way
static void seg_tables(const char *name, int64_t n_seg, int64_t n_items, bool pairs, size_t extra) {
    SegTables t, hit;
    Carve cv, again;
    pols::seg_tables_layout(cv, t, n_seg, n_items, pairs, extra);
    place(cv);
    fill(const_cast<int64_t *>(t.offs), 8 * (pairs ? 2 * n_seg : n_seg + 1)); fill(const_cast<int32_t *>(t.map), 4 * n_seg);
    fill(const_cast<int32_t *>(t.first), 4 * (n_items + 1)); fill(t.extra, extra * n_seg);
    pols::seg_tables_layout(again, hit, n_seg, n_items, pairs, extra);
    again.place(g_base);
    std::printf("%s %ld %ld %ld %ld %zu %ld %ld %ld %ld %zu\n", name, off(t.offs), off(t.map), off(t.first), off(t.extra), cv.total(), off(hit.offs),
                off(hit.map), off(hit.first), off(hit.extra), again.total());
}

// the LDS layout of a one-wave solve kernel (fit_lds.hpp): "lds <name> : <offset of every area, in the struct's order> <total>", in doubles
template <int N>
static void lds_line(const char *name, const int (&offs)[N]) {
    std::printf("lds %s :", name);
    for (int v : offs) std::printf(" %d", v);
    std::printf("\n");
}
static void lds_layouts() {
    char name[64];
    for (int k = 1; k <= 31; ++k) {
        const pols::AbsorbLds a = pols::k16_lds(k), b = pols::k17_lds(k);
        std::snprintf(name, sizeof name, "k16_%d", k);
        lds_line(name, {a.Gs, a.T, a.A, a.d0, a.rhs, a.Ri, a.total});
        std::snprintf(name, sizeof name, "k17_%d", k);
        lds_line(name, {b.Gs, b.T, b.A, b.d0, b.rhs, b.Ri, b.total});
        const pols::K18Lds c = pols::k18_lds(k);
        std::snprintf(name, sizeof name, "k18_%d", k);
        lds_line(name, {c.Ss, c.Cs, c.z1, c.zn, c.Gm, c.A, c.rhs, c.d0, c.b0, c.vv, c.tn, c.td, c.Ri, c.ij, c.total});
    }
    // K14: (kx, L, T) -- every kx with one endogenous column and one instrument, then wider instrument lists up to the cap T = 31
    auto k14 = [&](int kx, int L, int T) {
        const pols::K14Lds d = pols::k14_lds(kx, L, T);
        std::snprintf(name, sizeof name, "k14_%d_%d_%d", kx, L, T);
        lds_line(name, {d.Gs, d.A, d.d0, d.B, d.Gm2, d.A2, d.rhs2, d.d02, d.Ri, d.tmp, d.total});
    };
    for (int kx = 1; kx <= 30; ++kx) k14(kx, kx, kx + 1);
    k14(6, 8, 10); k14(2, 29, 30); k14(30, 31, 31); k14(15, 16, 31);
}

int main() {
    lds_layouts();
    enet_gram("enet_split", 37, 5, 45, true);
    enet_gram("enet_whole", 5, 5, 45, false);
    {   // an absent region without a stand-in (K17's group list of a frame that is not mixed), between two present ones
        uint32_t *ord = nullptr, *pos = nullptr;
        int32_t stale = 0, *list = &stale;
        Carve cv;
        cv.add(ord, 4 * 1001 + 4); cv.add(list, 0); cv.add(pos, 4 * 1001 + 4);
        place(cv);
        fill(ord, 4 * 1001 + 4); fill(pos, 4 * 1001 + 4);
        std::printf("absent %ld %ld %ld %zu\n", off(ord), off(list), off(pos), cv.total());
    }
    {   // a repeat: K16's category tables once per id column (items = 7, N = 415)
        int32_t *cnt[2] = {}, *idx[2] = {};
        int64_t *first[2] = {};
        Carve cv;
        for (int w = 0; w < 2; ++w) { cv.add(cnt[w], 4 * 7); cv.add(first[w], 8 * (7 + 1)); cv.add(idx[w], 4 * 415 + 4); }
        place(cv);
        for (int w = 0; w < 2; ++w) { fill(cnt[w], 4 * 7); fill(first[w], 8 * 8); fill(idx[w], 4 * 415 + 4); }
        std::printf("repeat %ld %ld %ld %ld %ld %ld %zu\n", off(cnt[0]), off(first[0]), off(idx[0]), off(cnt[1]), off(first[1]), off(idx[1]), cv.total());
    }
    {   // the same two sizes twice in sequence: K17's means and their weight sums (kz = 5, 33 and 12 categories)
        double *am1 = nullptr, *am2 = nullptr, *aw1 = nullptr, *aw2 = nullptr;
        const size_t b1 = 8 * 5 * 33 + 8, b2 = 8 * 5 * 12 + 8;
        Carve cv;
        cv.add(am1, b1); cv.add(am2, b2); cv.add(aw1, b1); cv.add(aw2, b2);
        place(cv);
        fill(am1, b1); fill(am2, b2); fill(aw1, b1); fill(aw2, b2);
        std::printf("twice %ld %ld %ld %ld %zu\n", off(am1), off(am2), off(aw1), off(aw2), cv.total());
    }
    {   // a raw region the entry lays out itself (K12: 100 doubles, then 100 int32), an exact multiple of 256 behind it, a const slot
        char *packed = nullptr;
        double *exact = nullptr;
        const double *ro = nullptr;
        Carve cv;
        cv.add(packed, 8 * 100 + 4 * 100); cv.add(exact, 512); cv.add(ro, 1);
        place(cv);
        fill(packed, 1200); fill(exact, 512);
        std::printf("raw %ld %ld %ld %zu\n", off(packed), off(exact), off(ro), cv.total());
    }
    kept("kept_all", 15); kept("kept_mid", 1 | 4 | 8); kept("kept_end", 1 | 2); kept("kept_none", 0);
    {   // a fixed pad in front of and behind a region: flag words on a line of their own, the pad that ends a table
        double *mid = nullptr;
        Carve cv;
        cv.gap(256); cv.add(mid, 8 * 33); cv.gap(256);
        place(cv);
        fill(mid, 8 * 33);
        std::printf("gap %ld %zu\n", off(mid), cv.total());
    }
    {   // a run of equal columns is one region (5 columns of 415 floats, each on its own 256-byte line); an empty frame's column still has an address
        char *cols = nullptr, *none = nullptr;
        const size_t stride = Carve::round(4 * 415);
        Carve cv;
        cv.add(cols, stride * 5); cv.keep(none, 0);
        place(cv);
        for (size_t j = 0; j < 5; ++j) fill(pols::column(cols, stride, j), 4 * 415);
        const float *ro = reinterpret_cast<const float *>(cols);
        std::printf("columns %ld %ld %ld %ld %ld %zu\n", off(pols::column(cols, stride, 0)), off(pols::column(cols, stride, 3)),
                    off(pols::column(cols, stride, 4)), off(pols::column(ro, stride, 2)), off(none), cv.total());
    }
    chunk_tables("chunks_plain", 5, 37, 9000, false, false);
    chunk_tables("chunks_host_valid", 5, 37, 9000, true, false);
    chunk_tables("chunks_device_valid", 5, 37, 9000, true, true);
    seg_tables("seg_frame", 40, 4, false, 8 * 17);
    seg_tables("seg_classes", 40, 3, true, 8 * 17);
    std::free(g_base);
    // the groups K17 keeps resident: all, none, mixed with an empty group, cap = -1 (the global route for every group, the empty one too)
    const int64_t offs[] = {0, 60, 260, 260, 7860, 7980}, full[] = {0, 60, 260, 7860};
    const struct { const int64_t *offs; size_t G; int64_t cap; } frames[] = {{offs, 5, 10000}, {full, 3, 10}, {offs, 5, 200}, {offs, 5, -1}};
    for (const auto &f : frames) {
        const pols::K17Split s = pols::k17_split_groups(f.offs, f.G, f.cap);
        std::printf("split %lld %lld %lld :", (long long)s.n_res, (long long)s.max_res, (long long)s.max_glb);
        for (int32_t g : s.list) std::printf(" %d", g);
        std::printf("\n");
    }
    return 0;
}
