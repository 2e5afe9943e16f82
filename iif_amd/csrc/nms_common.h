// What the NMS files share (nms.hip, multiclass_nms.hip): the order-preserving float key, the sort-key layout
// score bits << 24 | ~index, mmcv's overlap test and the pieces of the radix select.
#pragma once
#include "common.h"

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kSelThreads = 1024;             // the selection passes: thread t owns bins 4 t .. 4 t + 3
constexpr int kBins = 4096;
constexpr int kPasses = 5;                    // digits of 12, 12, 12, 12, 8 bits
constexpr u32 kIndexMask = 0xFFFFFFu;

struct SelState { u64 prefix; u32 rem; u32 pad; };

// bits that order as unsigned integers the way the floats order; -0 and +0 are one value
__device__ __forceinline__ u32 fkey(float f) {
    u32 u = __float_as_uint(f);
    if (f == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(u32 k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ __forceinline__ u32 wave_max_u(u32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u32 t = (u32)__shfl_xor((int)v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// mmcv nms_cuda_kernel.cuh: S = (x2 - x1 + offset) * (y2 - y1 + offset); p suppresses q (or q p: every step is symmetric) when
// inter / (Sp + Sq - inter) > thr.  Single float32 operations in mmcv's order (-ffp-contract=off); a NaN quotient does not suppress.
__device__ __forceinline__ float nms_area(const f32x4 p, float off) { return (p.z - p.x + off) * (p.w - p.y + off); }
__device__ __forceinline__ bool nms_suppresses(const f32x4 p, float sp, const f32x4 q, float sq, float off, float thr) {
    const float left = fmaxf(p.x, q.x), right = fminf(p.z, q.z);
    const float top = fmaxf(p.y, q.y), bottom = fminf(p.w, q.w);
    const float w = fmaxf(right - left + off, 0.0f), h = fmaxf(bottom - top + off, 0.0f);
    const float inter = w * h;
    const float iou = inter / (sp + sq - inter);
    return iou > thr;
}

__device__ __forceinline__ int digit_shift(int p) { return p < 4 ? 44 - 12 * p : 0; }
__device__ __forceinline__ int digit_bits(int p) { return p < 4 ? 12 : 8; }

// exclusive prefix sums over the block's 1024 threads; s_w: 17 words of LDS, reusable after the call returns
__device__ __forceinline__ u32 block_scan_excl(u32 v, u32* s_w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u32 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 t = (u32)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    if (wv == 0) {
        const u32 x = lane < kSelThreads / 64 ? s_w[lane] : 0u;
        u32 xi = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u32 t = (u32)__shfl_up((int)xi, o, 64);
            if (lane >= o) xi += t;
        }
        if (lane < kSelThreads / 64) s_w[lane] = xi - x;
    }
    __syncthreads();
    const u32 res = s_w[wv] + inc - v;
    __syncthreads();
    return res;
}
