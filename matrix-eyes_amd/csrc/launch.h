// Host side of a persistent kernel's launch: the dynamic-LDS attribute, the occupancy query and the grid (launch_grid.h has the
// arithmetic).  The hipLaunchKernelGGL itself stays in the kernel's own launcher, whose argument list only it knows.
//
// The cache is one PerDeviceOnce per kernel INSTANTIATION, and the caller owns it: a `static PerDeviceOnce once;` inside the launcher
// template, beside the `auto kern = some_kernel<...>;` it belongs to, handed in with the kernel.  The helpers must not hold that static
// themselves behind a template on the kernel's function TYPE: every gemm_*_kernel<...> is a void(GemmParams), so all would share the first's.
#pragma once
#include "common.h"
#include "launch_grid.h"

namespace me {

// the dynamic LDS a kernel may ask for, on the current device ...
inline void set_max_dynamic_lds(const void* kern, int smem) { ME_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem)); }
// ... once per device, for a kernel whose grid is not sized from its occupancy (gemm_launch_ring, stereogram_launch)
inline void set_max_dynamic_lds_once(PerDeviceOnce& once, const void* kern, int smem) {
    per_device_once(once, [&](int) {
        set_max_dynamic_lds(kern, smem);
        return 1;  // (configured)
    });
}

// Workgroups of `kern` (threads per workgroup, smem bytes of dynamic LDS; smem > 0 also sets the attribute) resident at once on the device,
// or on the cu_granted CUs the launch stream may use (0: all).  Asked once per device, cached as (workgroups per CU) << 12 | CUs.
inline int kernel_resident(PerDeviceOnce& once, const void* kern, int threads, int smem, int cu_granted = 0) {
    const int occ = per_device_once(once, [&](int dev) {
        if (smem > 0) set_max_dynamic_lds(kern, smem);
        int per_cu = 0, cus = 0;
        ME_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, smem));
        ME_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        return ((per_cu < 1 ? 1 : per_cu) << 12) | (cus < 1 ? 1 : (cus > 4095 ? 4095 : cus));
    });
    return resident_workgroups(occ >> 12, occ & 4095, cu_granted);
}

// The grid of a persistent launch of `kern` over ntiles tiles; `what` ("gemm", "conv", ...) names the launcher in the errors.
// The arguments behind it are the two-group launchers' (gemm_launch_pp, gemm_fp8.hip launch_pp8t): GemmParams::cu_granted,
// GemmParams::resident_out -- the query form: the resident count goes there and 0 comes back, there is nothing to launch --,
// the fused LayerNorm's round, gemm_grid_limit() and GemmParams::grid_cap (launch_grid.h persistent_grid).
inline unsigned persistent_launch_grid(PerDeviceOnce& once, const void* kern, int threads, int smem, int64_t ntiles, const char* what,
                                       int cu_granted = 0, int32_t* resident_out = nullptr, int64_t ln_unit = 0, int limit = 0, int cap = 0) {
    const int resident = kernel_resident(once, kern, threads, smem, cu_granted);
    if (resident_out) {
        *resident_out = resident;
        return 0;
    }
    ME_CHECK(ntiles > 0 && ntiles < (1ll << 31), ME_ERR_BAD_SHAPE, "%s grid %lld out of range", what, (long long)ntiles);
    const int64_t grid = persistent_grid(ntiles, resident, ln_unit, limit, cap);
    // (pipeline.hip ln_fusable asks gemm_lnf_resident / gemm_fp8_lnf_resident first and takes the stand-alone LayerNorm otherwise)
    ME_CHECK(grid > 0, ME_ERR_HIP, "%s: the fused LayerNorm needs %lld resident workgroups (%d fit)", what, (long long)ln_unit, resident);
    return (unsigned)grid;
}

}  // namespace me
