// The block-wide exclusive scan of the selection kernels (nms_common.h, sample_core.h, roi_stage.hip), once.
#pragma once
#include "common.h"

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kSelThreads = 1024;             // the block size the scan and every select built on it are written for

// Exclusive prefix sums over the block's kSelThreads threads.  W is u32, or u64 holding two 32-bit counts (neither half reaches
// 2^31).  s_w: kSelThreads / 64 + 1 words of LDS, reusable after the call returns; `total`, if given, receives the block's sum.
template <class W>
__device__ __forceinline__ W block_scan_excl(W v, W* s_w, W* total = nullptr) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    W inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const W t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    if (wv == 0) {
        const W x = lane < kSelThreads / 64 ? s_w[lane] : W(0);
        W xi = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const W t = __shfl_up(xi, o, 64);
            if (lane >= o) xi += t;
        }
        if (lane < kSelThreads / 64) s_w[lane] = xi - x;
        if (total && lane == 63) s_w[kSelThreads / 64] = xi;
    }
    __syncthreads();
    const W res = s_w[wv] + inc - v;
    if (total) *total = s_w[kSelThreads / 64];
    __syncthreads();
    return res;
}
