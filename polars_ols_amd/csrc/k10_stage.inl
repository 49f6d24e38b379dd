// k10_stage.inl -- the tile staging of K10 (k10_ridge_path.hip), shared with K11 (k11_rlm.hip): 256 rows of the columns go to LDS as f64
// with the null policy and sqrt(w) applied.  16-byte loads on the columns' 16-byte grid (column q of the tile is one wave's work, every
// load of a lane issued before the first use), then one thread per row applies the policy.
#pragma once
#include "common.hpp"

namespace pols {

constexpr int K10_TILE = 256;         // rows of a tile: one per thread

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
