// carve_check.cpp -- csrc/scratch_carve.hpp and csrc/k17_split.hpp on the CPU (no HIP): test_scratch_carve_cpu.py compiles this with
// -fsanitize=address,undefined, runs it and compares every printed line with formulas written out by hand.  Each scenario carves a heap
// buffer of exactly total() bytes and writes every region end to end, so a region that reaches past the total is a sanitizer report.
// Output: "<scenario> <offset of every slot, -1 for nullptr> ... <total>"; "split <n_res> <max_res> <max_glb> : <list>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "k17_split.hpp"
#include "scratch_carve.hpp"

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

int main() {
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
