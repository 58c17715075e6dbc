// ring_scan.h -- the 64-bit integer prefix sums that kernels_rings.hip and kernels_simplify.hip share: within a wave, and over an
// array by one 256-thread block.
#pragma once
#include "common.h"

namespace stcd {

__device__ __forceinline__ long long rg_wave_scan(long long v, int lane) {      // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// one block: a[stride * i] becomes the sum of the entries before i; returns the total (to every thread)
__device__ __forceinline__ long long rg_block_scan(long long* __restrict__ a, int64_t n, int stride, long long* ws) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    long long carry = 0;
    for (int64_t base = 0; base < n; base += 256) {                    // uniform
        const int64_t i = base + threadIdx.x;
        const long long v = i < n ? a[stride * i] : 0;
        const long long inc = rg_wave_scan(v, lane);
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) before += ws[w]; total += ws[w]; }
        if (i < n) a[stride * i] = carry + before + inc - v;
        carry += total;
        __syncthreads();                                               // ws is written again
    }
    return carry;
}

}  // namespace stcd
