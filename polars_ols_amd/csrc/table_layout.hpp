// table_layout.hpp -- the layouts of the two cached device tables that are read back on a cache hit: each is ONE function, called when
// the table is built (its total sizes the allocation) and when it is found again (the same slots over the kept buffer), so the two views
// cannot drift apart.  Plain C++ (no HIP): tests/carve_check.cpp checks both on the CPU.
#pragma once

#include <cstdint>

#include "scratch_carve.hpp"

// Long groups cut into segments (ensure_segments, api_internal.hpp): segment offsets, segment -> item, item -> first segment, then
// `extra_per_seg` bytes per segment for the caller's partial results.
struct SegTables {
    const int64_t *offs = nullptr;
    const int32_t *map = nullptr, *first = nullptr;
    int64_t n_seg = 0, max_len = 0, max_seg = 0;      // rows of the longest segment; most segments of one group
    char *extra = nullptr;
};

namespace pols {

// pairs: the tables of a size class hold a (start, end) pair per segment, those of the whole frame n_seg + 1 offsets
static inline void seg_tables_layout(Carve &cv, SegTables &t, int64_t n_seg, int64_t n_items, bool pairs, size_t extra_per_seg) {
    cv.keep(t.offs, sizeof(int64_t) * (size_t)(pairs ? 2 * n_seg : n_seg + 1));
    cv.keep(t.map, sizeof(int32_t) * (size_t)n_seg);
    cv.keep(t.first, sizeof(int32_t) * (size_t)(n_items + 1));
    cv.keep(t.extra, extra_per_seg * (size_t)n_seg);
    t.n_seg = n_seg;
}

// The tables of the chunk-parallel dynamic kernels (build_chunk_tables): groups and chunks (records of `group_bytes` / `chunk_bytes`),
// the work order, then -- only with validity bytes -- the prefix tables cnt / vidx, then -- only when those are built on the device --
// the slab counts, slab bases and compacted offsets of that pass; a pad of 256 bytes ends the table.
struct ChunkTables {
    char *groups = nullptr, *chunks = nullptr;
    int32_t *order = nullptr, *cnt = nullptr, *vidx = nullptr;
    uint32_t *slab_cnt = nullptr;
    int64_t *slab_base = nullptr, *c_offs = nullptr;
};
static inline void chunk_tables_layout(Carve &cv, ChunkTables &t, size_t group_bytes, size_t chunk_bytes, int64_t n_groups, int64_t n_chunks,
                                int64_t n_rows, bool prefix, bool on_device) {
    const int64_t n_slabs = (n_rows + 255) / 256;
    cv.keep(t.groups, group_bytes * (size_t)n_groups);
    cv.keep(t.chunks, chunk_bytes * (size_t)n_chunks);
    cv.keep(t.order, sizeof(int32_t) * (size_t)n_chunks);
    if (prefix) {
        cv.keep(t.cnt, sizeof(int32_t) * (size_t)n_rows);
        cv.keep(t.vidx, sizeof(int32_t) * (size_t)n_rows);
    }
    if (on_device) {
        cv.keep(t.slab_cnt, sizeof(uint32_t) * (size_t)n_slabs);
        cv.keep(t.slab_base, sizeof(int64_t) * (size_t)(n_slabs + 1));
        cv.keep(t.c_offs, sizeof(int64_t) * (size_t)(n_groups + 1));
    }
    cv.gap(256);
}

}  // namespace pols
