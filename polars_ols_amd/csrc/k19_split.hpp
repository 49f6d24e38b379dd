// k19_split.hpp -- which groups K19's resident table kernel takes: those whose rows of the category table number at most `cap`
// (cap < 0: none).  A pure function of the groups' table rows on the host (plain C++, no HIP: tests/k19_layout_check.cpp checks it on
// the CPU).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace pols {

struct K19Split {
    int64_t n_res = 0, n_glb = 0, max_res = 0;       // the resident groups, the others, the longest resident table
    std::vector<int32_t> list;                       // a mixed frame only: the resident groups, then the others
    bool mixed() const { return !list.empty(); }
};

inline K19Split k19_split_groups(const int64_t *rows, size_t G, int64_t cap) {
    K19Split s;
    for (size_t g = 0; g < G; ++g) {
        if (rows[g] <= cap) { ++s.n_res; s.max_res = std::max(s.max_res, rows[g]); } else ++s.n_glb;
    }
    if (s.n_res == 0 || s.n_glb == 0) return s;
    s.list.resize(G);
    size_t ir = 0, ig = (size_t)s.n_res;
    for (size_t g = 0; g < G; ++g) s.list[rows[g] <= cap ? ir++ : ig++] = (int32_t)g;
    return s;
}

}  // namespace pols
