// k7c_cluster.hpp -- K7c: one- and two-way cluster-robust standard errors of mode="statistics" (pols_least_squares_statistics_cluster).
#pragma once
#include "k7_stats.hpp"

namespace pols {

constexpr int K7C_TILE = 256;   // positions per LDS tile of the scores kernel (one per thread)

struct ClusterArgs {
    StatsArgs s;              // the K7 arguments of the same call: staged columns, offsets, Gram matrices, segment tables (seg_offs == nullptr:
                              // one segment per group); s.se / s.tv / s.pv receive the cluster-robust standard errors, t- and p-values
    int64_t n_rows;
    int32_t ways;             // 1 (ids[0]) or 2 (ids[0], ids[1])
    int32_t use_correction;   // G / (G - 1) (N - 1) / df per clustering
    const int64_t *ids[2];    // device, one per row in the batch's row order
    int64_t *n_clusters;      // device, n_groups x ways, or nullptr
    double *prep;             // n_groups x k7r_prep_stride(kt): A^-1, b, trace(A^-1), ok                           (Work::ClusterPrep)
    double *part;             // (segments or groups) x k7c_part_stride(kt), then 3 x n_groups x (kt + 1) sums     (Work::ClusterPart)
};

// One clustering (A, B or the pairs AB) as the scores / finish kernels see it.
struct ClusterWay {
    const uint32_t *order;    // position -> row: every group's positions in ascending id order, frame order within an id; nullptr = identity
    const int64_t *k1, *k2;   // the id columns whose change starts a cluster (k2: the second id of AB, else nullptr)
    double *part;             // per segment / group: sum z^2 of the runs inside, the pieces cut by its ends, counts and flags
    double *sums;             // n_groups x (kt + 1): sum_c z_cj^2 (j < kt), G
};

// per segment: [sum z^2: kt][head piece H: kt][tail piece T: kt][run starts][head open][head closes here][tail open]
__host__ __device__ inline size_t k7c_part_stride(int kt) { return 3 * (size_t)kt + 4; }

// prepare (K7r's) / per clustering: runs, scores, finish / se, t, p on the stream; r2 / mae / mse come from K7 unchanged
int k7c_cluster_launch(pols_ctx *ctx, int dtype, const ClusterArgs &c);

// the runs step alone, for one id column (device, one id per row): *order = position -> row with every group's positions in ascending
// id order and frame order within an id (Work::ClusterSort / ClusterOrder, valid until the next call that orders), or nullptr when
// the probe found the ids non-decreasing inside every group already.  Synchronises the stream once (the probe's result).
int k7c_order_launch(pols_ctx *ctx, const int64_t *ids, const int64_t *offs, int64_t n_groups, int64_t n_rows, const uint32_t **order);

// out[w][i] = in[w][src[i]] for the ways id columns: the ids of the rows a null policy keeps (src: row_compact_srcmap_launch)
int k7c_gather_ids_launch(pols_ctx *ctx, const int32_t *src, int64_t n, const int64_t *const *in, int64_t *const *out, int ways);

}  // namespace pols
