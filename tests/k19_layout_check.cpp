// k19_layout_check.cpp -- K19's LDS layout (csrc/fit_lds.hpp: k19_lds, k19_resident_rows) and its split of the groups into the two routes of
// the table kernel (csrc/k19_split.hpp) on the CPU (no HIP): test_random_effects_layout_cpu.py compiles this with the address and
// undefined-behaviour sanitizers, runs it and compares what it prints with sizes written out by hand.  Every area is written end to end
// into a buffer of exactly the total, so an area that reaches past it is a sanitizer report.
// Output: "lds <k> <kc> <rows> : <offset of every area, in the struct's order> <total>", "cap <k> <kc> <budget> : <rows>",
// "split <n_res> <n_glb> <max_res> : <list>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fit_lds.hpp"
#include "k19_split.hpp"

static void lds_line(int k, int kc, int rows) {
    const pols::K19Lds o = pols::k19_lds(k, kc, rows);
    const int offs[] = {o.tab, o.q, o.part, o.Gw, o.Gs, o.T, o.A, o.d0, o.rhs, o.Ri, o.Minv, o.bb, o.D, o.dz, o.dv, o.red, o.sc, o.total};
    const int n = (int)(sizeof offs / sizeof offs[0]);
    std::vector<double> buf((size_t)o.total);
    for (int i = 0; i + 1 < n; ++i)
        for (int at = offs[i]; at < offs[i + 1]; ++at) buf[(size_t)at] += 1.0;         // every double belongs to exactly one area
    for (int at = 0; at < o.total; ++at)
        if (buf[(size_t)at] != 1.0) { std::printf("overlap at %d\n", at); std::exit(1); }
    std::printf("lds %d %d %d :", k, kc, rows);
    for (int i = 0; i < n; ++i) std::printf(" %d", offs[i]);
    std::printf("\n");
}

static void cap_line(int k, int kc, long long budget) {
    const long long rows = pols::k19_resident_rows(k, kc, budget);
    std::printf("cap %d %d %lld : %lld\n", k, kc, budget, rows);
    if (rows > 0) {                                                // the capacity fits the budget, one row more does not
        const long long fits = 8LL * pols::k19_lds(k, kc, (int)rows).total, over = 8LL * pols::k19_lds(k, kc, (int)rows + 1).total;
        if (fits > budget || over <= budget) { std::printf("capacity off: %lld %lld\n", fits, over); std::exit(1); }
    }
}

static void split_line(const std::vector<int64_t> &rows, int64_t cap) {
    const pols::K19Split s = pols::k19_split_groups(rows.data(), rows.size(), cap);
    std::printf("split %lld %lld %lld :", (long long)s.n_res, (long long)s.n_glb, (long long)s.max_res);
    for (int32_t g : s.list) std::printf(" %d", (int)g);
    std::printf("\n");
}

int main() {
    for (int k = 1; k <= 31; ++k)
        for (int icpt = 0; icpt < 2 && k + icpt <= 31; ++icpt) {
            lds_line(k, k + icpt, 0);
            lds_line(k, k + icpt, 15);
        }
    lds_line(8, 9, 1000);
    const long long budget = 160 * 1024 - 256;
    cap_line(2, 3, budget);
    cap_line(8, 9, budget);
    cap_line(30, 31, budget);
    cap_line(30, 31, 1024);                                        // a budget below the fixed part: nothing is resident
    const std::vector<int64_t> rows = {15, 200, 0, 12000, 40};
    split_line(rows, 20000);                                       // all resident, no list
    split_line(rows, 10);                                          // only the empty group fits
    split_line(rows, 200);                                         // mixed: the resident groups first
    split_line(rows, -1);                                          // the forced global route: not even the empty group
    split_line({}, 100);
    return 0;
}
