// phj_wave.h — sums and scans over the 64 lanes of a wave and the kWaves waves
// of a kBlock workgroup (every lane of the wave / thread of the workgroup calls).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "phj_partition.h"

namespace phj {

// The wave's sum of x, in lane 0.
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}

// Inclusive scan: the sum of x over lanes 0..lane.
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= static_cast<uint32_t>(o)) x += y;
    }
    return x;
}

// The workgroup's sum of x, returned to thread 0 (0 elsewhere); red: LDS.
template <class T>
__device__ __forceinline__ T block_sum(T x, T (&red)[kWaves]) {
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    T t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kWaves; w++) t += red[w];
    return t;
}

}  // namespace phj
