// Grid arithmetic of the persistent kernels (GEMM, convolution, attention), free of HIP so that a host compiler alone can
// build and test it (tests/test_launch_grid_cpu.py).  launch.h has the HIP side.
#pragma once
#include <stdint.h>

namespace me {

// Workgroups resident at once: per_cu (the occupancy API's answer; at least 1) on each of the device's `cus` compute units, or on the
// cu_granted a stream with a CU mask may use when that is fewer (0: no mask).  Whole XCD rounds -- workgroup b lands on XCD b % 8 --, at least one.
inline int resident_workgroups(int per_cu, int cus, int cu_granted) {
    if (per_cu < 1) per_cu = 1;
    if (cu_granted > 0 && cu_granted < cus) cus = cu_granted;
    int r = per_cu * cus;
    r -= r % 8;
    return r < 8 ? 8 : r;
}

// Workgroups of a persistent launch over ntiles tiles: no more than there are tiles, no more than are resident.
//   unit > 0   the fused residual + LayerNorm launch (gemm_core.h resid_ln_epilogue): whole rounds of unit = 8 * N / BN workgroups, a
//              row tile per XCD with all its column tiles, all resident because they wait for one another.  -1 when resident < unit:
//              the caller raises, nothing may be launched.
//   limit >= 8 at most that many, in whole XCD rounds (gemm_grid_limit()); on a LayerNorm launch it may split a round: that is its use.
//   cap >= 8   the same for GemmParams::grid_cap; a LayerNorm launch ignores it.
inline int64_t persistent_grid(int64_t ntiles, int resident, int64_t unit, int limit, int cap) {
    int64_t g = ntiles < resident ? ntiles : resident;
    if (unit > 0) {
        if (resident < unit) return -1;
        g -= g % unit;
    }
    if (limit >= 8 && g > limit) g = limit - limit % 8;
    if (unit == 0 && cap >= 8 && g > cap) g = cap - cap % 8;
    return g;
}

}  // namespace me
