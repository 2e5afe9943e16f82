// The two ends of the Mask R-CNN mask branch for gfx950 (MI355X): both are a bilinear resampling of a one-channel image between
// a box and a fixed grid, bounded by one pass over bytes, ending in a threshold.
//
//   iif_mask_targets   instance_segmentation/mmdet/core/mask/mask_target.py:7-127 with BitmapMasks.crop_and_resize
//                      (core/mask/structures.py:333-367): clip the proposal to the image, mmcv's RoIAlign (spatial_scale 1,
//                      sampling_ratio 0, aligned, 'avg') on the gt mask the index names, >= 0.5 - for all images in ONE launch.
//   iif_paste_masks    models/roi_heads/mask_heads/fcn_mask_head.py:179-310, 344-412: class channel, sigmoid, _do_paste_mask's
//                      grid, grid_sample (bilinear, align_corners=False, zero padding), >= threshold - in ONE launch.
//
// iif_mask_targets.  A block is (roi, slab of output rows); a roi whose clipped box is less than 2 * kSlabPx pixels high
// uses one block, taller ones up to kSlabs (the other blocks of its grid row return after the geometry).  The bin is summed in the separable form of roi_align.hip with the shared helpers
// of roi_geom.h:  bin = sum_y Wy[ph][y] * (sum_x Wx[pw][x] * m[y, x]) / count.  The per-axis weights Wx are built once per block
// (one compact run of pixels per bin, roi_w + 3 MW floats at most).  Mask rows then stream through LDS a few at a time: each wave
// takes a row, its lanes run along x - a scalar head up to the first 16-byte boundary of the row's ADDRESS, 16-byte loads, a scalar
// tail, because W, the pitch and the clipped box start are arbitrary; the LDS row keeps the address's misalignment so the 16-byte
// LDS stores are aligned as well.  Every mask byte inside the clipped box is read from memory once per roi (rows shared by two
// slabs: once per slab).  From LDS, work item (row, bin[, part]) forms  R[y][pw] = sum_x Wx[pw][x] [m != 0]  over the bin's run,
// then item (ph, pw) adds  Wy[ph][y] * R[y][pw]  in ascending y.  This one form serves both regimes: with bins of many pixels a
// run is long and is cut into up to 8 parts on neighbouring lanes (a fixed butterfly adds them); with bins below one pixel a run
// is one or two pixels and the same pixel feeds many bins - out of LDS, so it still costs one global read.  No atomics: the
// result does not depend on timing, on the slab count or on where the mask lies in memory.
//
// iif_paste_masks.  A block is (detection, band of image rows).  The [h, w] class channel goes through the sigmoid into LDS once
// per block that needs it.  Output bytes are produced over the band's FLAT byte range: a scalar head to the first 16-byte
// boundary of the address, 16 pixels per 16-byte store, a scalar tail (img_w is arbitrary, so rows start anywhere).  A
// conservative pixel rectangle around the box (two pixels and a tap's reach wider than where any tap can land) lets chunks, rows
// and whole bands outside it be written as the constant  0 >= threshold  without touching LDS or computing a coordinate; inside
// it every pixel evaluates the reference's float32 expressions in their order and decides by the taps themselves.  The pixel's
// definition lives in mask_paste.h, which mask_rle.hip (the same masks as COCO run lengths, without the image) shares.
#include "common.h"
#include "roi_geom.h"
#include "mask_paste.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / IIF_WAVE;

// ---------------------------------------------------------------------------------------------------------------- mask targets
constexpr int kMaxImages = 16;
constexpr int kMaxOut = 64;                   // MH, MW
constexpr int kMaxW = 4096;                   // mask width: the per-axis weights of a whole-image box live in LDS
constexpr int kWxCap = kMaxW + 3 * kMaxOut + 64;
constexpr int kTileBytes = 16384;
constexpr int kTY = 16;                       // mask rows per pass at most
constexpr int kSlabs = 8;
constexpr int kSlabPx = 64;
constexpr int kMaxGrid = 65536;               // as roi_align.hip

struct MaskImages {
    const uint8_t* p[kMaxImages];
    int64_t ld_row[kMaxImages], ld_mask[kMaxImages];
    int G[kMaxImages], H[kMaxImages], W[kMaxImages];
};

struct TargetArgs {
    MaskImages im;
    int B, MH, MW, binarize;
    const float* rois; int64_t ld; const int64_t* gt; int64_t K;
    float* out;
};

struct TGeom {
    bool skip;
    int img, H, W, grid_h, grid_w;
    int64_t g;
    float start_h, start_w, bin_h, bin_w, count, roi_h;
};

// Everything that depends on the roi alone: mask_target_single's np.clip on the float32 proposal, then mmcv's roi geometry at
// spatial_scale 1, aligned.  Uniform over the block.
__device__ __forceinline__ TGeom target_geometry(const TargetArgs& a, int64_t k) {
    TGeom g;
    const float* r = a.rois + k * a.ld;
    const float b = r[0];
    float x1 = r[1], y1 = r[2], x2 = r[3], y2 = r[4];
    g.skip = !(b >= 0.0f && b < (float)a.B) || !finite_f(x1) || !finite_f(y1) || !finite_f(x2) || !finite_f(y2);
    g.img = g.skip ? 0 : (int)b;
    g.H = a.im.H[g.img]; g.W = a.im.W[g.img];
    g.g = a.gt[k];
    if (g.g < 0 || g.g >= (int64_t)a.im.G[g.img]) g.skip = true;
    const float fw = (float)g.W, fh = (float)g.H;
    x1 = fminf(fmaxf(x1, 0.0f), fw); x2 = fminf(fmaxf(x2, 0.0f), fw);
    y1 = fminf(fmaxf(y1, 0.0f), fh); y2 = fminf(fmaxf(y2, 0.0f), fh);
    g.start_w = x1 * 1.0f - 0.5f; g.start_h = y1 * 1.0f - 0.5f;
    const float end_w = x2 * 1.0f - 0.5f, end_h = y2 * 1.0f - 0.5f;
    const float roi_w = end_w - g.start_w, roi_h = end_h - g.start_h;
    g.roi_h = roi_h;
    g.bin_h = roi_h / (float)a.MH;
    g.bin_w = roi_w / (float)a.MW;
    const float gh = ceilf(roi_h / (float)a.MH), gw = ceilf(roi_w / (float)a.MW);
    if (!(gh <= (float)kMaxGrid && gw <= (float)kMaxGrid)) g.skip = true;
    g.grid_h = g.skip ? 0 : (int)gh;
    g.grid_w = g.skip ? 0 : (int)gw;
    const int64_t cnt = (int64_t)g.grid_h * g.grid_w;
    g.count = (float)(cnt > 1 ? cnt : 1);
    return g;
}

__device__ __forceinline__ unsigned misalign16(const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u); }

__global__ void __launch_bounds__(kThreads) mask_targets_kernel(TargetArgs a) {
    __shared__ float wxs[kWxCap];                               // Wx, one run per bin
    __shared__ __align__(16) uint8_t tile[kTileBytes];          // the mask rows of one pass
    __shared__ float rsum[kTY * kMaxOut];                       // R[row][pw]
    __shared__ float wyt[kMaxOut * kTY];                        // Wy[ph of the slab][row of the pass]
    __shared__ float acc[kMaxOut * kMaxOut];
    __shared__ int xlo[kMaxOut], xlen[kMaxOut], xoff[kMaxOut], ylo[kMaxOut], yhi[kMaxOut];
    __shared__ int sh[4];
    const int tid = threadIdx.x;
    const int lane = tid & (IIF_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t k = blockIdx.x;
    const int s = blockIdx.y;
    const int MH = a.MH, MW = a.MW;
    float* out = a.out + k * MH * MW;
    const TGeom g = target_geometry(a, k);
    if (g.skip || g.grid_h <= 0 || g.grid_w <= 0) {
        if (s == 0)
            for (int e = tid; e < MH * MW; e += kThreads) out[e] = 0.0f;
        return;
    }
    // the slab count comes from the clipped height alone (at most H here), so a surplus slab returns before any LDS work
    const int nsl = max(1, min((int)g.roi_h / kSlabPx, min((int)gridDim.y, MH)));
    if (s >= nsl) return;
    if (tid < MH) {
        int lo, hi;
        if (!axis_range(g.start_h, g.bin_h, g.grid_h, tid, g.H, &lo, &hi)) { lo = 0; hi = -1; }
        ylo[tid] = lo; yhi[tid] = hi;
    }
    if (tid >= IIF_WAVE && tid < IIF_WAVE + MW) {
        int lo, hi;
        if (!axis_range(g.start_w, g.bin_w, g.grid_w, tid - IIF_WAVE, g.W, &lo, &hi)) { lo = 0; hi = -1; }
        xlo[tid - IIF_WAVE] = lo; xlen[tid - IIF_WAVE] = hi - lo + 1;
    }
    __syncthreads();
    if (tid == 0) {
        int x0 = INT32_MAX, x1 = -1, off = 0;
        for (int pw = 0; pw < MW; ++pw) {
            xoff[pw] = off;
            off += xlen[pw];
            if (xlen[pw] > 0) { x0 = min(x0, xlo[pw]); x1 = max(x1, xlo[pw] + xlen[pw] - 1); }
        }
        sh[1] = off; sh[2] = x0; sh[3] = x1;
    }
    __syncthreads();
    const int total = sh[1], X0 = sh[2], X1 = sh[3];
    const int ph0 = s * MH / nsl, ph1 = (s + 1) * MH / nsl, nph = ph1 - ph0;
    int Y0 = INT32_MAX, Y1 = -1;
    for (int ph = ph0; ph < ph1; ++ph)
        if (yhi[ph] >= ylo[ph]) { Y0 = min(Y0, ylo[ph]); Y1 = max(Y1, yhi[ph]); }
    const int span = X1 - X0 + 1;
    // total <= kWxCap and span <= kMaxW always hold: a run is [floor(first sample), floor(last sample) + 1] and the samples of a
    // bin lie less than bin_w apart, so a run has at most bin_w + 3 pixels and the MW runs roi_w + 3 MW <= W + 3 MW <= kWxCap in all
    // (the entry refuses W > kMaxW, MW > kMaxOut); the comparison only keeps an LDS index in range should that reasoning ever break
    if (Y1 < Y0 || X1 < X0 || total > kWxCap || span > kMaxW) {
        for (int e = tid; e < nph * MW; e += kThreads) out[ph0 * MW + e] = 0.0f;
        return;
    }
    for (int pw = 0; pw < MW; ++pw)
        for (int j = tid; j < xlen[pw]; j += kThreads)
            wxs[xoff[pw] + j] = axis_weight(g.start_w, g.bin_w, g.grid_w, pw, g.W, xlo[pw] + j);
    for (int e = tid; e < nph * MW; e += kThreads) acc[e] = 0.0f;
    const int pitch = (span + 15 + 15) & ~15;                   // a row keeps its address's misalignment (< 16)
    const int TY = min(kTY, kTileBytes / pitch);
    int parts = 1;                                               // a bin's run is cut into `parts` (1, 2, 4, 8): about 8 pixels each
    while (parts < 8 && span > MW * 8 * parts) parts *= 2;
    const uint8_t* base = a.im.p[g.img] + g.g * a.im.ld_mask[g.img] + X0;
    const int64_t ldr = a.im.ld_row[g.img];
    __syncthreads();
    for (int y0 = Y0; y0 <= Y1; y0 += TY) {
        const int ny = min(TY, Y1 - y0 + 1);
        for (int r = wave; r < ny; r += kWaves) {
            const uint8_t* src = base + (int64_t)(y0 + r) * ldr;
            const int mis = (int)misalign16(src);
            uint8_t* dst = tile + r * pitch + mis;
            const int head = min((16 - mis) & 15, span);
            if (lane < head) dst[lane] = src[lane];
            const int nvec = (span - head) >> 4;
            for (int v = lane; v < nvec; v += IIF_WAVE)
                *reinterpret_cast<u32x4*>(dst + head + 16 * v) = *reinterpret_cast<const u32x4*>(src + head + 16 * v);
            const int t0 = head + 16 * nvec;
            if (t0 + lane < span) dst[t0 + lane] = src[t0 + lane];
        }
        for (int e = tid; e < nph * ny; e += kThreads) {
            const int phl = e / ny, r = e - phl * ny, ph = ph0 + phl, y = y0 + r;
            wyt[phl * kTY + r] = (y >= ylo[ph] && y <= yhi[ph]) ? axis_weight(g.start_h, g.bin_h, g.grid_h, ph, g.H, y) : 0.0f;
        }
        __syncthreads();
        const int items = ny * MW * parts;
        for (int e0 = 0; e0 < items; e0 += kThreads) {           // whole waves run the shuffles: items past the end sum nothing
            const int e = e0 + tid;
            const int part = e & (parts - 1), q = e / parts;
            const int r = q / MW, pw = q - r * MW;
            float sum = 0.0f;
            if (e < items) {
                const int len = xlen[pw], per = (len + parts - 1) / parts;
                const int j0 = min(part * per, len), j1 = min(j0 + per, len);
                const uint8_t* t = tile + r * pitch + (int)misalign16(base + (int64_t)(y0 + r) * ldr) + (xlo[pw] - X0);
                const float* w = wxs + xoff[pw];
                for (int j = j0; j < j1; ++j)
                    if (t[j]) sum += w[j];
            }
            for (int o = 1; o < parts; o <<= 1) sum += __shfl_xor(sum, o, IIF_WAVE);
            if (e < items && part == 0) rsum[r * kMaxOut + pw] = sum;
        }
        __syncthreads();
        for (int e = tid; e < nph * MW; e += kThreads) {
            const int phl = e / MW, pw = e - phl * MW;
            float v = acc[e];
            for (int r = 0; r < ny; ++r) {
                const float w = wyt[phl * kTY + r];
                if (w != 0.0f) v += w * rsum[r * kMaxOut + pw];
            }
            acc[e] = v;
        }
        __syncthreads();
    }
    for (int e = tid; e < nph * MW; e += kThreads) {
        const float v = acc[e] / g.count;
        out[ph0 * MW + e] = a.binarize ? (v >= 0.5f ? 1.0f : 0.0f) : v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- paste
constexpr int kBandBytes = 65536;

struct PasteArgs {
    const void* pred; int dtype, activated;
    const int64_t* labels;
    const float* boxes; int64_t ldb;
    int C, h, w, img_h, img_w, rows_per_band;
    float thr;
    uint8_t* out;
};

__global__ void __launch_bounds__(kThreads) paste_masks_kernel(PasteArgs a) {
    __shared__ float tile[kMaxPred * kMaxPred];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.y;
    const int yb0 = (int)blockIdx.x * a.rows_per_band;
    const int yb1 = min(a.img_h, yb0 + a.rows_per_band);
    PasteBox b;
    int64_t c;
    const bool valid = paste_box(a.boxes + n * a.ldb, a.labels, n, a.C, a.h, a.w, a.img_h, a.img_w, a.thr, &b, &c);
    b.any = valid && b.xhi >= b.xlo && !(b.yhi < yb0 || b.ylo >= yb1);
    if (b.any) {
        const int hw = a.h * a.w;
        paste_load_tile(a.pred, a.dtype, a.activated, (n * a.C + c) * hw, hw, tile, tid, kThreads);
        __syncthreads();
    }
    const int64_t img0 = n * a.img_h * a.img_w;
    const int64_t f0 = img0 + (int64_t)yb0 * a.img_w, f1 = img0 + (int64_t)yb1 * a.img_w;
    uint8_t* o = a.out;
    const int64_t hb0 = (16 - (int64_t)misalign16(o + f0)) & 15, hb = hb0 < f1 - f0 ? hb0 : f1 - f0;
    if (tid < hb) {
        const int rel = (int)(f0 + tid - img0), y = rel / a.img_w;
        o[f0 + tid] = paste_pixel(b, tile, y, rel - y * a.img_w);
    }
    const int64_t nchunk = (f1 - f0 - hb) >> 4;
    const unsigned fill4 = b.fill * 0x01010101u;
    for (int64_t ch = tid; ch < nchunk; ch += kThreads) {
        const int64_t fb = f0 + hb + 16 * ch;
        const int rel = (int)(fb - img0);
        int y = rel / a.img_w, x = rel - y * a.img_w;
        u32x4 v = {fill4, fill4, fill4, fill4};
        const bool one_row = x + 15 < a.img_w;
        if (b.any && !(one_row && (y < b.ylo || y > b.yhi || x + 15 < b.xlo || x > b.xhi))) {
            unsigned wds[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned word = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    word |= (unsigned)paste_pixel(b, tile, y, x) << (8 * i);
                    if (++x == a.img_w) { x = 0; ++y; }
                }
                wds[q] = word;
            }
            v = u32x4{wds[0], wds[1], wds[2], wds[3]};
        }
        *reinterpret_cast<u32x4*>(o + fb) = v;
    }
    const int64_t tb = f0 + hb + 16 * nchunk;
    if (tb + tid < f1) {
        const int rel = (int)(tb + tid - img0), y = rel / a.img_w;
        o[tb + tid] = paste_pixel(b, tile, y, rel - y * a.img_w);
    }
}

}  // namespace

extern "C" {

int iif_mask_targets(const iif_mask_image* images, int num_images, const float* rois, int64_t ld_rois, const int64_t* gt_inds,
                     int64_t K, int mask_h, int mask_w, int binarize, float* out, void* stream) {
    if (!images || num_images < 1 || num_images > kMaxImages || K < 0 || K > INT32_MAX || ld_rois < 5) return IIF_EINVAL;
    if (mask_h <= 0 || mask_w <= 0) return IIF_EINVAL;
    if (mask_h > kMaxOut || mask_w > kMaxOut) return IIF_EUNSUPPORTED;
    TargetArgs a{};
    for (int i = 0; i < num_images; ++i) {
        const iif_mask_image& m = images[i];
        if (m.G < 0 || m.H <= 0 || m.W <= 0 || (m.G > 0 && !m.ptr)) return IIF_EINVAL;
        if (m.ld_row < m.W || m.ld_mask < (int64_t)(m.H - 1) * m.ld_row + m.W) return IIF_EINVAL;
        if (m.W > kMaxW) return IIF_EUNSUPPORTED;
        a.im.p[i] = m.ptr; a.im.G[i] = m.G; a.im.H[i] = m.H; a.im.W[i] = m.W; a.im.ld_row[i] = m.ld_row; a.im.ld_mask[i] = m.ld_mask;
    }
    if (K == 0) return IIF_OK;
    if (!rois || !aligned_to(rois, 4) || !gt_inds || !aligned_to(gt_inds, 8) || !out || !aligned_to(out, 4)) return IIF_EINVAL;
    a.B = num_images; a.MH = mask_h; a.MW = mask_w; a.binarize = binarize != 0;
    a.rois = rois; a.ld = ld_rois; a.gt = gt_inds; a.K = K; a.out = out;
    hipLaunchKernelGGL(mask_targets_kernel, dim3((unsigned)K, kSlabs), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_paste_masks(const void* mask_pred, int dtype, int activated, const int64_t* labels, const float* boxes, int64_t ld_boxes,
                    int64_t N, int C, int h, int w, int img_h, int img_w, float threshold, uint8_t* out, void* stream) {
    if (N < 0 || N > 65535 || C <= 0 || h <= 0 || w <= 0 || img_h <= 0 || img_w <= 0 || ld_boxes < 4) return IIF_EINVAL;
    if (dtype != IIF_F32 && dtype != IIF_BF16) return IIF_EINVAL;
    if (!(threshold >= 0.0f)) return IIF_EINVAL;                        // negative (the uint8 visualisation branch) or NaN
    if (h > kMaxPred || w > kMaxPred || (int64_t)img_h * img_w > INT32_MAX) return IIF_EUNSUPPORTED;
    if (N == 0) return IIF_OK;
    if (!mask_pred || !aligned_to(mask_pred, dtype == IIF_BF16 ? 2 : 4) || !boxes || !aligned_to(boxes, 4) || !out) return IIF_EINVAL;
    if (labels && !aligned_to(labels, 8)) return IIF_EINVAL;
    PasteArgs a{};
    a.pred = mask_pred; a.dtype = dtype; a.activated = activated != 0; a.labels = labels; a.boxes = boxes; a.ldb = ld_boxes;
    a.C = C; a.h = h; a.w = w; a.img_h = img_h; a.img_w = img_w; a.thr = threshold; a.out = out;
    a.rows_per_band = kBandBytes / img_w > 1 ? kBandBytes / img_w : 1;
    const unsigned bands = (unsigned)cdiv64(img_h, a.rows_per_band);
    hipLaunchKernelGGL(paste_masks_kernel, dim3(bands, (unsigned)N), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // extern "C"
