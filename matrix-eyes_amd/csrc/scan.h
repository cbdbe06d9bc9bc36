// The prefix sums of the device-side byte-stream producers (OBJ text, PNG deflate, JPEG decode and encode, mesh indexing),
// once: a wave scan, a workgroup scan on top of it, the two kernels built from that and their launches.  Device only.
// Everything here combines integers with an associative operation, so a result never depends on the order of the steps.
#pragma once
#include "common.h"

namespace me_scan {

struct Plus {
    template <class T> __device__ T operator()(const T& a, const T& b) const { return a + b; }
};

// the value of the lane d below (d above for Down = true), dword by dword; lanes without such a lane keep their own
template <bool Down = false, class T> __device__ __forceinline__ T lane_shift(const T& v, int d) {
    static_assert(sizeof(T) % 4 == 0, "shuffled as dwords");
    uint32_t w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k) w[k] = Down ? __shfl_down(w[k], d, 64) : __shfl_up(w[k], d, 64);
    T r;
    __builtin_memcpy(&r, w, sizeof(T));
    return r;
}

// inclusive scan over the wave's 64 lanes: lane l gets op(v[0], ..., v[l]).  Every lane of the wave must be here.
template <class T, class Op = Plus> __device__ __forceinline__ T wave_scan(T v, Op op = Op()) {
    const int lane = (int)threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T left = lane_shift(v, d);
        if (lane >= d) v = op(left, v);
    }
    return v;
}

// the sum over the wave's 64 lanes, in lane 0
template <class T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += lane_shift<true>(v, d);
    return v;
}

// Exclusive scan over a workgroup of THREADS threads: returns op(v[0], ..., v[t - 1]) (T() for thread 0, which must be
// op's identity) and sets `total` to the workgroup's in every thread.  `totals` is LDS of the caller's; one barrier, so
// a caller that uses `totals` again puts a barrier of its own in between.
template <int THREADS, class T, class Op = Plus>
__device__ __forceinline__ T block_scan(const T& v, T (&totals)[THREADS / 64], T& total, Op op = Op()) {
    static_assert(THREADS % 64 == 0, "whole waves");
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const T incl = wave_scan(v, op);
    if (lane == 63) totals[wave] = incl;
    __syncthreads();
    T before = T(), all = T();
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        const T tw = totals[w];
        if (w < wave) before = op(before, tw);
        all = op(all, tw);
    }
    total = all;
    const T below = lane_shift(incl, 1);
    return lane == 0 ? before : op(before, below);
}

// a struct -> its copy in LDS, as dwords by the whole workgroup; ends with a barrier
template <int THREADS, class T> __device__ __forceinline__ void stage_to_lds(T& lds, const T* g) {
    static_assert(sizeof(T) % 4 == 0, "copied as dwords");
    const uint32_t* src = reinterpret_cast<const uint32_t*>(g);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&lds);
    for (int k = (int)threadIdx.x; k < (int)(sizeof(T) / 4); k += THREADS) dst[k] = src[k];
    __syncthreads();
}

// before[i]: the sum of counts[j] over the j < i of i's workgroup; agg[g]: workgroup g's sum
template <int THREADS>
__global__ __launch_bounds__(THREADS) void scan_groups_kernel(const uint32_t* __restrict__ counts, int64_t n,
                                                              uint64_t* __restrict__ before, uint64_t* __restrict__ agg) {
    __shared__ uint64_t totals[THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * THREADS + (int)threadIdx.x;
    uint64_t total;
    const uint64_t excl = block_scan<THREADS>((uint64_t)(i < n ? counts[i] : 0), totals, total);
    if (i < n) before[i] = excl;
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// out[i]: base + the sum of in[0 .. i); out[n]: base + the total.  One workgroup: a thread sums a slice of the input, the
// slices' sums are scanned, and the thread walks its slice again.
template <int THREADS, class In>
__global__ __launch_bounds__(THREADS) void scan_slices_kernel(const In* __restrict__ in, int64_t n, uint64_t base,
                                                              uint64_t* __restrict__ out) {
    __shared__ uint64_t totals[THREADS / 64];
    const int tid = (int)threadIdx.x;
    const int64_t per = (n + THREADS - 1) / THREADS;
    const int64_t lo = (int64_t)tid * per < n ? (int64_t)tid * per : n, hi = lo + per < n ? lo + per : n;
    uint64_t mine = 0;
    for (int64_t i = lo; i < hi; ++i) mine += in[i];
    uint64_t total;
    uint64_t run = base + block_scan<THREADS>(mine, totals, total);
    for (int64_t i = lo; i < hi; ++i) {
        out[i] = run;
        run += in[i];
    }
    if (tid == 0) out[n] = base + total;
}

// one workgroup: n counts -> n + 1 offsets from `base`
template <int THREADS, class In> void launch_offsets(const In* in, int64_t n, uint64_t base, uint64_t* out, hipStream_t s) {
    hipLaunchKernelGGL((scan_slices_kernel<THREADS, In>), dim3(1), dim3(THREADS), 0, s, in, n, base, out);
    ME_HIP(hipGetLastError());
}

// two levels: the offset of i is before[i] + carry[i / THREADS], carry[ceil(n / THREADS)] the total; n > 0
template <int THREADS>
void launch_two_level(const uint32_t* counts, int64_t n, uint64_t* before, uint64_t* agg, uint64_t* carry, hipStream_t s) {
    const int64_t ngroups = me::cdiv(n, THREADS);
    hipLaunchKernelGGL(scan_groups_kernel<THREADS>, dim3((unsigned)ngroups), dim3(THREADS), 0, s, counts, n, before, agg);
    ME_HIP(hipGetLastError());
    launch_offsets<THREADS>((const uint64_t*)agg, ngroups, 0, carry, s);
}

}  // namespace me_scan
