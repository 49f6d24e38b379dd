// k9_sort.hpp -- K9's device-wide stable radix sort (rocPRIM) on buffers the caller owns: used by the group-key ingestion
// (k9_layout.hip) and by the cluster runs of the cluster-robust statistics (k7c_cluster.hip).
#pragma once
#include "common.hpp"

namespace pols {

// Stable LSD sort of n (key, value) pairs on the key bits [0, bits): keys_out / vals_out in ascending key order, equal keys in
// their input order.  tmp == nullptr: *tmp_bytes receives the temporary storage the call needs; nothing runs.  U: uint32_t, uint64_t.
template <typename U>
int k9_radix_sort_pairs(pols_ctx *ctx, void *tmp, size_t *tmp_bytes, const U *keys_in, U *keys_out, const uint32_t *vals_in,
                        uint32_t *vals_out, int64_t n, int bits);

}  // namespace pols
