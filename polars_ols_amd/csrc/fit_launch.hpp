// fit_launch.hpp -- the host side of a launch of the per-group fit kernels K10 .. K14 and K16 .. K18 (the device side: fit_tile.inl,
// fit_solve.inl, fit_group.inl).
#pragma once
#include "common.hpp"

namespace pols {

constexpr size_t FIT_LDS_BUDGET = 160 * 1024 - 256;   // dynamic LDS a launch may ask for

// workgroups of a launch over the frame: one per segment of a long group (ensure_segments) or one per group
template <typename Args>
inline int64_t fit_items(const Args &a) { return a.seg_offs ? a.n_seg : a.n_groups; }

// raises the kernel's dynamic-LDS limit to `budget` once per device (once: the launcher's own mask)
template <typename K>
int fit_raise_lds(pols_ctx *ctx, K kernel, OncePerDevice &once, const size_t budget) {
    if (once.needed(ctx->device)) {
        POLS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)budget));
        once.done(ctx->device);
    }
    return POLS_OK;
}

// ... and launches it
template <typename K, typename... A>
int fit_launch(pols_ctx *ctx, K kernel, OncePerDevice &once, const int64_t grid, const int block, const size_t lds, const size_t budget,
               const A &...args) {
    const int rc = fit_raise_lds(ctx, kernel, once, budget);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), lds, ctx->stream, args...);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

// the plain launch of a kernel whose LDS stays under the default limit (the one-wave-per-group kernels): nothing for an empty grid
template <typename K, typename... A>
static inline int fit_launch_plain(pols_ctx *ctx, K kernel, const int64_t grid, const int block, const size_t lds, const A &...args) {
    if (grid == 0) return POLS_OK;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), lds, ctx->stream, args...);
    POLS_HIP(hipGetLastError());
    return POLS_OK;
}

}  // namespace pols
