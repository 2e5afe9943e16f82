// The per-axis RoIAlign geometry (mmcv's, pool_mode 'avg') that roi_align.hip and mask_ops.hip share: the float32 sample
// coordinate in the reference's order, the pixel range the kept samples of one bin touch, and the summed weight of one pixel -
// the separable form documented at the head of roi_align.hip.  Host and device; the build passes -ffp-contract=off.
#pragma once
#include "common.h"

namespace {

__host__ __device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }     // false for NaN and +-inf


__host__ __device__ __forceinline__ float sample_coord(float start, float bin, int p, int i, float fgrid) {
    return start + (float)p * bin + ((float)i + 0.5f) * bin / fgrid;
}

// Pixel range [lo, hi] of one axis of one bin that the kept samples can touch; false: none.  The sample coordinate is monotone
// in i (every float32 step of it is), so the first and the last sample bound the rest.
__host__ __device__ __forceinline__ bool axis_range(float start, float bin, int grid, int p, int size, int* lo, int* hi) {
    const float fg = (float)grid;
    const float ya = sample_coord(start, bin, p, 0, fg), yb = sample_coord(start, bin, p, grid - 1, fg);
    const float mn = fminf(ya, yb), mx = fmaxf(ya, yb);
    const float top = (float)(size - 1);
    if (mx < -1.0f || mn > (float)size) return false;
    *lo = (int)fminf(fmaxf(floorf(mn), 0.0f), top);
    *hi = (int)fminf(fmaxf(floorf(mx) + 1.0f, 0.0f), top);
    return true;
}

// W[pix] of one axis of one bin (see the head of the file); pix differs per lane
__host__ __device__ __forceinline__ float axis_weight(float start, float bin, int grid, int p, int size, int pix) {
    const float fg = (float)grid;
    float w = 0.0f;
    for (int i = 0; i < grid; ++i) {
        float y = sample_coord(start, bin, p, i, fg);
        if (y < -1.0f || y > (float)size) continue;
        if (y <= 0.0f) y = 0.0f;
        int lo = (int)y, hi;
        if (lo >= size - 1) {
            hi = lo = size - 1;
            y = (float)lo;
        } else {
            hi = lo + 1;
        }
        const float l = y - (float)lo, h = 1.0f - l;
        if (lo == pix) w += h;
        if (hi == pix) w += l;
    }
    return w;
}

}  // namespace
