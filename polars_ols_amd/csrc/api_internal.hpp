// api_internal.hpp -- what the entry translation units (api.hip, api_fits.hip) share beyond common.hpp; all of it is defined in api.hip.
#pragma once

#include <vector>

#include "common.hpp"

namespace pols {

int check_ctx(pols_ctx *ctx);
int check_batch(const pols_batch *b, const pols_out *o, int max_features = POLS_MAX_FEATURES);
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Host-resident batch: stage every column into device scratch (PCIe-inclusive path).
struct Staged {
    const void *y = nullptr, *w = nullptr;
    const uint8_t *valid = nullptr;
    std::vector<const void *> x;     // n_features column pointers (device)
    void *coef = nullptr, *pred = nullptr, *resid = nullptr;
    int32_t *status = nullptr;
};

int stage_inputs(pols_ctx *ctx, const pols_batch *b, int64_t coef_rows, int kt, const pols_out *o, Staged *st);
int unstage_outputs(pols_ctx *ctx, const pols_batch *b, int64_t coef_rows, int kt, const pols_out *o, const Staged &st);
int fill_null_weights(pols_ctx *ctx, const pols_batch *b, Staged *st);

}  // namespace pols

// Long groups cut into segments (the streamed static path, the statistics of long groups): a group is one workgroup in those
// kernels, so ONE regression over a 10M-row frame used to be one CU's work.  Groups longer than two segments are cut into pieces
// of about N / (8 x CUs) rows (256-row multiples), the others are one segment each; tables in ctx->seg_cache -- segment offsets,
// segment -> group, group -> first segment -- followed by `extra_per_seg` bytes per segment for the caller's partial results.
// n_seg = 0: nothing is longer than two segments (or POLS_NO_SPLIT).  Cached per frame.
struct SegTables {
    const int64_t *offs = nullptr;
    const int32_t *map = nullptr, *first = nullptr;
    int64_t n_seg = 0, max_len = 0, max_seg = 0;      // rows of the longest segment; most segments of one group
    char *extra = nullptr;
};
// ids (size classes): the tables cover only the listed groups (ascending), `offs` holds (start, end) PAIRS per segment, `map` gives the segment's
// position in the list and `first` is indexed by list position; class_key tells such tables apart in the cache (0 = the whole frame).
int ensure_segments(pols_ctx *ctx, const pols_batch *b, int64_t max_rows, size_t extra_per_seg, SegTables *t,
                    const std::vector<int32_t> *ids = nullptr, int64_t class_key = 0);
