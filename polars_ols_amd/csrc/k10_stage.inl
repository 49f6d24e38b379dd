// k10_stage.inl -- the tile staging of K10 (k10_ridge_path.hip), shared with K11 (k11_rlm.hip) and K14 (k14_iv.hip): 256 rows of the columns go to LDS as f64
// with the null policy and sqrt(w) applied.  16-byte loads on the columns' 16-byte grid (column q of the tile is one wave's work, every
// load of a lane issued before the first use), then one thread per row applies the policy.
#pragma once
#include "common.hpp"

namespace pols {

constexpr int K10_TILE = 256;         // rows of a tile: one per thread
constexpr int K10_GRAM_TS = 257;      // column stride of a tile whose columns are read across threads (odd: conflict-free across columns)

// the item of this workgroup: its group, its rows, and the first row of its tile grid (the columns' 16-byte grid).  Args: as k10_stage,
// and offs, seg_offs, seg_map.
template <typename T, typename Args>
__device__ __forceinline__ void k10_item(const Args &a, int64_t &g, int64_t &s, int64_t &e, int64_t &base, int64_t &ntiles) {
    const int64_t sgi = blockIdx.x;
    g = a.seg_offs ? (int64_t)a.seg_map[sgi] : sgi;
    s = a.seg_offs ? a.seg_offs[sgi] : a.offs[g];
    e = a.seg_offs ? a.seg_offs[sgi + 1] : a.offs[g + 1];
    base = s & ~(int64_t)(Vec16<T>::N - 1);
    ntiles = e > s ? (e - base + K10_TILE - 1) / K10_TILE : 0;
}

// the entries of a symmetric nz x nz cross-product that thread `tid` of 256 accumulates: (ei, ej) of slot q, ei <= ej, in the order of
// the packed upper triangle.  With ne = nz (nz + 1) / 2 < 256 entries `parts` = 256 / ne row partitions share an entry (slot 0 only,
// this thread's partition is `part`), beyond that up to three entries per thread (parts = 1).
__device__ __forceinline__ void k10_entries(const int nz, const int parts, const int part, int (&ei)[3], int (&ej)[3], bool (&on)[3]) {
    const int tid = threadIdx.x, ne = nz * (nz + 1) / 2;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int en = parts > 1 ? tid - part * ne : tid + 256 * q;
        on[q] = parts > 1 ? (q == 0 && part < parts) : en < ne;
        int i = 0, t = on[q] ? en : 0;
        while (t >= nz - i) { t -= nz - i; ++i; }
        ei[q] = i; ej[q] = i + t;
    }
}

// rows [t0, t0 + 256) of the item [s, e) into xs (column stride ts): features 0 .. ku - 1, the ones column at ku (kt > ku), y~ at kt;
// column kt + 1 holds the raw weights in between.  Args: RidgeCvArgs (K10) or RlmArgs (K11) -- y, w, x, n_rows, valid, null_policy, k_user, kt.  Returns whether this thread's row (t0 + tid) is a fitted row.  Ends on a barrier.
template <typename T, bool STREAM, typename Args>
__device__ __forceinline__ bool k10_stage(const Args &a, const int64_t s, const int64_t e, const int64_t t0, double *xs, const int ts) {
    using V = typename Vec16<T>::type;
    constexpr int VEC = Vec16<T>::N, CH = K10_TILE / VEC;
    const int tid = threadIdx.x, ku = a.k_user, kt = a.kt;
    const int nld = ku + 1 + (a.w ? 1 : 0);
    for (int p = tid; p < nld * CH; p += 256) {
        const int q = __builtin_amdgcn_readfirstlane(p / CH), ch = p - q * CH;     // (CH is 64 or 128: a wave stays inside one column)
        const int64_t row0 = t0 + (int64_t)ch * VEC;
        if (row0 >= e) continue;
        const void *col = q == ku ? a.y : a.w;                       // (a run-time index into the kernel arguments would put them in scratch)
#pragma unroll
        for (int j = 0; j < POLS_MAX_FEATURES; ++j) col = (j == q && j < ku) ? a.x[j] : col;
        const T *src = static_cast<const T *>(col);
        double *dst = xs + (size_t)(q < ku ? q : (q == ku ? kt : kt + 1)) * ts + ch * VEC;
        if (row0 + VEC <= a.n_rows) {                              // (the columns are 16-byte aligned and row0 sits on their grid)
            const V v = STREAM ? load_stream(reinterpret_cast<const V *>(src + row0)) : *reinterpret_cast<const V *>(src + row0);
#pragma unroll
            for (int i = 0; i < VEC; ++i) dst[i] = (double)vget<T>(v, i);
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) dst[i] = row0 + i < a.n_rows ? (double)src[row0 + i] : 0.0;
        }
    }
    __syncthreads();
    const int64_t row = t0 + tid;
    const int pol = a.null_policy;
    bool fit = row >= s && row < e;
    if (fit && pol != POLS_NULL_IGNORE) {                          // which rows leave the fit (compute_is_valid_mask, ex.rs:201-228)
        if (a.valid && null_checks_y(pol)) fit = a.valid[row] != 0;
        if (null_checks_y(pol)) { const double v = xs[(size_t)kt * ts + tid]; fit = fit && v == v; }
        if (null_checks_x(pol))
            for (int c = 0; c < ku; ++c) { const double v = xs[(size_t)c * ts + tid]; fit = fit && v == v; }
    }
    const double sw = !fit ? 0.0 : (a.w ? sqrt(xs[(size_t)(kt + 1) * ts + tid]) : 1.0);
    for (int c = 0; c < ku; ++c) {
        double v = xs[(size_t)c * ts + tid];
        if (pol != POLS_NULL_IGNORE && v != v) v = 0.0;           // handle_nulls (ex.rs:257-296)
        xs[(size_t)c * ts + tid] = fit ? v * sw : 0.0;
    }
    if (kt > ku) xs[(size_t)ku * ts + tid] = sw;
    {
        double v = xs[(size_t)kt * ts + tid];
        if (pol != POLS_NULL_IGNORE && v != v) v = 0.0;
        xs[(size_t)kt * ts + tid] = fit ? v * sw : 0.0;
    }
    __syncthreads();
    return fit;
}

}  // namespace pols
