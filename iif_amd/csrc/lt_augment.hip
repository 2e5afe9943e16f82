// List-dataset (ImageNet-LT / Places-LT / iNaturalist-18) training and evaluation input for gfx950 (MI355X): one launch builds
// a whole fp32 NCHW batch from host-cut uint8 source regions, in the order of TensorTransform (iif_amd/imbalanced_dataset.py) -
//   antialiased bilinear resize of the region to rh x rw, of which only the S x S window at (oy, ox) is formed
//   -> horizontal flip (descriptor bit)
//   -> [IIF_LT_JITTER] clamp to [0, 1], then brightness / contrast / saturation / hue in the drawn order (augment.ColorJitter)
//   -> (x - mean) / std.
//
// One 1024-thread block per image; thread t owns the output pixels p = t, t + 1024, ... (row p / S, column p % S), so a
// wave's 64 lanes read neighbouring source columns and write 64 consecutive floats of each channel plane.
//
// Resample: lt_resample.h (shared with lt_policy.hip).
//
// Contrast blends toward the mean of the grey image as it stands when contrast runs: a whole-image reduction.  The block
// makes two sweeps over its image when contrast is in the record.  The first resamples, applies the ops drawn before
// contrast, sums the grey values and parks the fp32 pixels in `out` (the same thread re-reads exactly what it wrote, so no
// fence beyond program order is needed); after one block-wide sum the second sweep reads them back, applies contrast and the
// later ops, normalises and overwrites them.  Without contrast (or with factor 1) one sweep does everything.
//
// Arithmetic: every colour op is augment.py's torch expression in fp32, operation by operation (-ffp-contract=off, IEEE
// division), with (f, 1 - f) rounded from double on the host as torch rounds the python scalar; the grey mean sums in double.
#include "lt_resample.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / IIF_WAVE;
constexpr unsigned kAllFlags = IIF_LT_JITTER;

// jitter record words (iif_amd/lt_device.py JITTER): order (2 bits per position), then fp32 bits
enum { J_ORDER, J_FB, J_GB, J_FC, J_GC, J_FS, J_GS, J_FH, J_WORDS };
enum { OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE };

struct LtArgs {
    const unsigned char* pool; int64_t pool_bytes;
    const int64_t* desc; const uint32_t* jitter;
    float* out; int S; unsigned flags;
    float mean[3], stdv[3];
};

// augment.adjust_hue: _rgb_to_hsv, H + shift mod 1, _hsv_to_rgb
__device__ void hue(float (&v)[3], float shift) {
    const float r = v[0], g = v[1], b = v[2];
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.0f : maxc);
    const float crd = eqc ? 1.0f : cr;
    const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
    const float hr = maxc == r ? bc - gc : 0.0f;
    const float hg = (maxc == g && maxc != r) ? 2.0f + rc - bc : 0.0f;
    const float hb = (maxc != g && maxc != r) ? 4.0f + gc - rc : 0.0f;
    float h = fmodf((hr + hg + hb) / 6.0f + 1.0f, 1.0f);
    h = fmodf(h + shift, 1.0f);                         // torch.remainder(., 1.0)
    if (h < 0.0f) h += 1.0f;
    const float fi = floorf(h * 6.0f);
    const float f = h * 6.0f - fi;
    const int i = (((int)fi % 6) + 6) % 6;
    const float vv = maxc;
    const float p = clamp01(vv * (1.0f - s));
    const float q = clamp01(vv * (1.0f - f * s));
    const float t = clamp01(vv * (1.0f - (1.0f - f) * s));
    switch (i) {
        case 0: v[0] = vv; v[1] = t; v[2] = p; break;
        case 1: v[0] = q; v[1] = vv; v[2] = p; break;
        case 2: v[0] = p; v[1] = vv; v[2] = t; break;
        case 3: v[0] = p; v[1] = q; v[2] = vv; break;
        case 4: v[0] = t; v[1] = p; v[2] = vv; break;
        default: v[0] = vv; v[1] = p; v[2] = q; break;
    }
}

// one colour op of the jitter record on one pixel (contrast takes the image mean as `m`)
__device__ __forceinline__ void colour_op(float (&v)[3], int op, const float (&k)[7], float m) {
    if (op == OP_BRIGHTNESS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = blend(v[c], 0.0f, k[0], k[1]);
    } else if (op == OP_CONTRAST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = blend(v[c], m, k[2], k[3]);
    } else if (op == OP_SATURATION) {
        const float gy = grey(v);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = blend(v[c], gy, k[4], k[5]);
    } else if (k[6] != 0.0f) {                          // adjust_hue skips a zero shift
        hue(v, k[6]);
    }
}

__device__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & (IIF_WAVE - 1)) == 0) red[threadIdx.x / IIF_WAVE] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) t += red[i];
    return t;
}

__global__ void __launch_bounds__(kThreads) lt_augment_kernel(LtArgs a) {
    __shared__ double red[kWaves];
    const int b = blockIdx.x;
    const int S = a.S, npix = S * S;
    float* out = a.out + (int64_t)b * 3 * npix;
    const int64_t* d = a.desc + (int64_t)b * D_WORDS;
    const int64_t off = d[D_OFF], h = d[D_H], w = d[D_W], rh = d[D_RH], rw = d[D_RW], oy = d[D_OY], ox = d[D_OX];
    const bool flip = d[D_FLIP] != 0;

    // a descriptor outside the pool or the resized image reads nothing: a zero image
    const bool ok = off >= 0 && h > 0 && w > 0 && h <= INT32_MAX && w <= INT32_MAX && w <= a.pool_bytes &&
                    h <= a.pool_bytes / (3 * w) && off <= a.pool_bytes - 3 * h * w && rh > 0 && rw > 0 &&
                    rh <= INT32_MAX && rw <= INT32_MAX && oy >= 0 && ox >= 0 && oy + S <= rh && ox + S <= rw;
    if (!ok) {
        for (int p = threadIdx.x; p < 3 * npix; p += kThreads) out[p] = 0.0f;
        return;
    }
    const unsigned char* src = a.pool + off;
    const float sy = (float)h / (float)rh, sx = (float)w / (float)rw;   // area_pixel_compute_scale: in / out in fp32

    const bool jit = a.flags & IIF_LT_JITTER;
    int order[4] = {0, 1, 2, 3};
    float k[7] = {1.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f};
    int cpos = 4;                                       // position of contrast in the order (4: no contrast sweep)
    if (jit) {
        const uint32_t* j = a.jitter + (int64_t)b * J_WORDS;
#pragma unroll
        for (int i = 0; i < 4; ++i) order[i] = (int)((j[J_ORDER] >> (2 * i)) & 3u);
#pragma unroll
        for (int i = 0; i < 7; ++i) k[i] = __uint_as_float(j[J_FB + i]);
        if (!(k[2] == 1.0f && k[3] == 0.0f))
#pragma unroll
            for (int i = 3; i >= 0; --i)
                if (order[i] == OP_CONTRAST) cpos = i;
    }

    double gsum = 0.0;
    for (int p = threadIdx.x; p < npix; p += kThreads) {
        const int y = p / S, x = p - y * S;
        float v[3];
        resample(src, (int)h, (int)w, sy, sx, (int)oy + y, (int)ox + (flip ? S - 1 - x : x), v);
        if (jit) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = clamp01(v[c]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < cpos) colour_op(v, order[i], k, 0.0f);
        }
        if (cpos < 4) {                                 // park the pre-contrast pixel; the finishing sweep reads it back
            gsum += (double)grey(v);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c * npix + p] = v[c];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c * npix + p] = (v[c] - a.mean[c]) / a.stdv[c];
        }
    }
    if (cpos == 4) return;

    const float m = (float)(block_sum(gsum, red) / (double)npix);
    for (int p = threadIdx.x; p < npix; p += kThreads) {
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = out[c * npix + p];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i >= cpos) colour_op(v, order[i], k, m);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c * npix + p] = (v[c] - a.mean[c]) / a.stdv[c];
    }
}

}  // namespace

extern "C" int iif_lt_augment(const uint8_t* pool, int64_t pool_bytes, const int64_t* desc, const uint32_t* jitter,
                              int64_t batch, int size, const float* mean_std, uint32_t flags, float* out, void* stream) {
    if (!pool || !desc || !mean_std || !out) return IIF_EINVAL;
    if (pool_bytes < 0 || batch < 0 || batch > INT32_MAX || size <= 0 || size > 16384 || (flags & ~kAllFlags)) return IIF_EINVAL;
    if ((flags & IIF_LT_JITTER) && !jitter) return IIF_EINVAL;
    if (batch == 0) return IIF_OK;
    LtArgs a{pool, pool_bytes, desc, jitter, out, size, flags, {}, {}};
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = mean_std[c];
        a.stdv[c] = mean_std[3 + c];
    }
    hipLaunchKernelGGL(lt_augment_kernel, dim3((unsigned)batch), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}
