// k17_split.hpp -- which groups K17's resident demean launch takes: those of at most `cap` rows (cap < 0: none).  A pure function of the
// host offsets (plain C++, no HIP: tests/carve_check.cpp checks it on the CPU).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace pols {

struct K17Split {
    int64_t n_res = 0, max_res = 0, max_glb = 0;     // the resident groups, their longest, the longest of the others
    std::vector<int32_t> list;                       // a mixed frame only: the resident groups, then the others
    bool mixed() const { return !list.empty(); }
};

inline K17Split k17_split_groups(const int64_t *offs, size_t G, int64_t cap) {
    K17Split s;
    for (size_t g = 0; g < G; ++g) {
        const int64_t rows = offs[g + 1] - offs[g];
        if (rows <= cap) { ++s.n_res; s.max_res = std::max(s.max_res, rows); } else s.max_glb = std::max(s.max_glb, rows);
    }
    if (s.n_res == 0 || (size_t)s.n_res == G) return s;
    s.list.resize(G);
    size_t ir = 0, ig = (size_t)s.n_res;
    for (size_t g = 0; g < G; ++g) s.list[(offs[g + 1] - offs[g] <= cap) ? ir++ : ig++] = (int32_t)g;
    return s;
}

}  // namespace pols
