// The pixel of a pasted mask, shared by mask_ops.hip (iif_paste_masks: the boolean image) and mask_rle.hip (iif_paste_rle_*: its
// COCO run lengths without the image): one definition, so both decide every pixel with the same bits.  Every step is the
// reference's float32 expression in its order (fcn_mask_head.py:344-412 with grid_sample; the build passes -ffp-contract=off).
#pragma once
#include "common.h"
#include "roi_geom.h"

namespace {

constexpr int kMaxPred = 64;                  // h, w of the predicted mask

// _do_paste_mask's normalised coordinate of pixel p on an axis with box edges (a, b), with its replacement of +-inf by 0
__device__ __forceinline__ float paste_coord(int p, float a, float b) {
    float v = ((float)p + 0.5f - a) / (b - a) * 2.0f - 1.0f;
    if (fabsf(v) > 3.402823466e38f) v = 0.0f;
    return v;
}

// grid_sample's source coordinate (align_corners=False)
__device__ __forceinline__ float paste_unnormalize(float v, int size) { return ((v + 1.0f) * (float)size - 1.0f) / 2.0f; }

// Pixels [lo, hi] outside which no tap of this axis can land inside the tile.  A tap lands inside for
// p in (a - .5 - d / 2size, b - .5 + d / 2size), d = b - a (mirrored for d < 0); the range returned is wider than that by more
// than 1.5 pixels, against float32 rounding of a few 2^-22 of the quantities involved.  Edges that are tiny, huge or not finite
// (where the reference's quotient may overflow to inf and be replaced by 0, i.e. land in the CENTRE of the tile): the whole axis.
__device__ __forceinline__ void paste_bounds(float a, float b, int size, int img, int* lo, int* hi) {
    *lo = 0; *hi = img - 1;
    const float ad = fabsf(b - a);
    if (finite_f(a) && finite_f(b) && ad >= 0.0009765625f && fabsf(a) <= 1048576.0f && fabsf(b) <= 1048576.0f) {
        const float m = ad / (float)size + 2.0f;
        const float flo = floorf(fminf(a, b) - m), fhi = ceilf(fmaxf(a, b) + m);
        *lo = max(0, (int)flo);
        *hi = min(img - 1, (int)fhi);
    }
}

struct PasteBox {
    float x0, y0, x1, y1, thr;
    int xlo, xhi, ylo, yhi, h, w;
    bool any;                                 // some pixel of this block may have a tap inside the tile (the tile is loaded)
    uint8_t fill;                             // every other pixel
};

__device__ __forceinline__ uint8_t paste_pixel(const PasteBox& b, const float* tile, int y, int x) {
    if (!b.any || y < b.ylo || y > b.yhi || x < b.xlo || x > b.xhi) return b.fill;
    const float ix = paste_unnormalize(paste_coord(x, b.x0, b.x1), b.w);
    const float iy = paste_unnormalize(paste_coord(y, b.y0, b.y1), b.h);
    if (!(ix > -1.0f && ix < (float)b.w && iy > -1.0f && iy < (float)b.h)) return b.fill;      // four taps outside (NaN too)
    const float fx = floorf(ix), fy = floorf(iy);
    const int xi = (int)fx, yi = (int)fy;
    const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
    const bool xa = xi >= 0, xb = xi + 1 < b.w, ya = yi >= 0, yb = yi + 1 < b.h;
    float v = 0.0f;
    if (ya && xa) v += tile[yi * b.w + xi] * (wx0 * wy0);
    if (ya && xb) v += tile[yi * b.w + xi + 1] * (wx1 * wy0);
    if (yb && xa) v += tile[(yi + 1) * b.w + xi] * (wx0 * wy1);
    if (yb && xb) v += tile[(yi + 1) * b.w + xi + 1] * (wx1 * wy1);
    return v >= b.thr ? 1 : 0;
}

// What of a detection does not depend on the block: the box, the conservative rectangle and the constant outside it.  Returns
// whether the label (*c; labels NULL: channel 0) names a channel; `any` is left to the caller (its block may lie outside the
// rectangle).
__device__ __forceinline__ bool paste_box(const float* bx, const int64_t* labels, int64_t n, int C, int h, int w, int img_h, int img_w,
                                          float thr, PasteBox* b, int64_t* c) {
    b->x0 = bx[0]; b->y0 = bx[1]; b->x1 = bx[2]; b->y1 = bx[3];
    b->thr = thr; b->h = h; b->w = w;
    *c = labels ? labels[n] : 0;
    const bool valid = *c >= 0 && *c < (int64_t)C;
    b->fill = (valid && 0.0f >= thr) ? 1 : 0;
    paste_bounds(b->x0, b->x1, w, img_w, &b->xlo, &b->xhi);
    paste_bounds(b->y0, b->y1, h, img_h, &b->ylo, &b->yhi);
    return valid;
}

// The [h, w] class channel at element offset `off` through the sigmoid (activated: as it is) into LDS; the caller synchronises.
__device__ __forceinline__ void paste_load_tile(const void* pred, int dtype, int activated, int64_t off, int hw, float* tile, int tid,
                                                int threads) {
    for (int e = tid; e < hw; e += threads) {
        float v = dtype == IIF_BF16 ? bf16_bits_to_f32(static_cast<const uint16_t*>(pred)[off + e])
                                    : static_cast<const float*>(pred)[off + e];
        if (!activated) v = 1.0f / (1.0f + expf(-v));
        tile[e] = v;
    }
}

}  // namespace
