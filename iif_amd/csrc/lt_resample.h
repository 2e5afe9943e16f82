// Pieces shared by the list-dataset input kernels (lt_augment.hip, lt_policy.hip): the descriptor words, ATen's antialiased bilinear resample of one output pixel, and the fp32 colour arithmetic of augment.py.
//
// Resample: interpolate(mode="bilinear", antialias=True, align_corners=False) as ATen's CPU kernel computes it, per axis:
// scale = in / out (fp32), support = max(scale, 1), centre = scale * (i + 0.5), taps [xmin, xmin + xsize) clipped to the
// region, triangle weights of (j + xmin - centre + 0.5) / max(scale, 1), renormalised by their sum.  The taps are evaluated
// in registers for each output pixel, for any scale: the cost is (taps in y) x (taps in x) per pixel, about 3 x 3 at
// ImageNet sizes.  Each row of taps is summed first (horizontal), then the rows (vertical), as ATen's separable passes do.
// The weights are not divided by their sum tap by tap: the unnormalised sum is divided by (sum_x * sum_y * 255) once,
// which also applies ToTensor's / 255 (a few ulp away from torch's order).
#pragma once
#include "common.h"

namespace {    // internal linkage in each kernel file, as if written there

// descriptor words (iif_amd/lt_device.py DESC)
enum { D_OFF, D_H, D_W, D_RH, D_RW, D_OY, D_OX, D_FLIP, D_WORDS };

// one axis of the antialiased resize at output coordinate i (ATen's _compute_indices_min_size_weights_aa; centre and window
// bounds rounded as its float / double mix does)
struct Taps {
    int xmin, xsize;
    float centre, invscale, total;
};

__device__ __forceinline__ float tri(float x) {
    x = fabsf(x);
    return x < 1.0f ? 1.0f - x : 0.0f;
}

__device__ __forceinline__ float tap_weight(const Taps& t, int j) {
    return tri(((float)(j + t.xmin) - t.centre + 0.5f) * t.invscale);
}

__device__ Taps taps(float scale, int in, int i) {
    Taps t;
    const float support = scale >= 1.0f ? scale : 1.0f;
    t.invscale = scale >= 1.0f ? (float)(1.0 / (double)scale) : 1.0f;
    t.centre = (float)((double)scale * ((double)i + 0.5));
    const int64_t lo = (int64_t)((double)(t.centre - support) + 0.5);
    const int64_t hi = (int64_t)((double)(t.centre + support) + 0.5);
    t.xmin = (int)(lo > 0 ? lo : 0);
    t.xsize = (int)((hi < in ? hi : in) - t.xmin);
    float tot = 0.0f;
    for (int j = 0; j < t.xsize; ++j) tot += tap_weight(t, j);
    t.total = tot;
    return t;
}

// the S x S window pixel (y, x) of the resized, flipped region, on [0, 1]
__device__ void resample(const unsigned char* src, int h, int w, float sy, float sx, int ry, int rx, float (&v)[3]) {
    const Taps ty = taps(sy, h, ry), tx = taps(sx, w, rx);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < ty.xsize; ++i) {
        const float wy = tap_weight(ty, i);
        const unsigned char* row = src + ((int64_t)(ty.xmin + i) * w + tx.xmin) * 3;
        float rs[3] = {0.0f, 0.0f, 0.0f};
        for (int j = 0; j < tx.xsize; ++j) {
            const float wx = tap_weight(tx, j);
#pragma unroll
            for (int c = 0; c < 3; ++c) rs[c] += wx * (float)row[3 * j + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += wy * rs[c];
    }
    const float tot = ty.total * tx.total;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = tot != 0.0f ? acc[c] / (tot * 255.0f) : 0.0f;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
// _blend: clamp(F x + G o, 0, 1) with F = f, G = 1 - f rounded from double on the host
__device__ __forceinline__ float blend(float x, float o, float F, float G) { return clamp01(F * x + G * o); }
__device__ __forceinline__ float grey(const float (&v)[3]) { return (0.2989f * v[0] + 0.587f * v[1]) + 0.114f * v[2]; }

}  // namespace
