// List-dataset (ImageNet-LT / Places-LT / iNaturalist-18) training input with an auto-augment policy, for gfx950 (MI355X):
// one launch builds a whole fp32 NCHW batch in the order of TensorTransform's training branch with ``auto_augment`` set
// (iif_amd/imbalanced_dataset.py) -
//   antialiased bilinear resize of the host-cut region, its S x S window, the flip (lt_resample.h; the same values as
//   iif_lt_augment) -> clamp to [0, 1] -> up to two auto-augment operations from the image's op record, in record order
//   -> (x - mean) / std.
// The host drew the sub-policy / RandAugment ops, their application and signs (iif_amd/lt_device.py policy_record); each
// record slot holds an op code (the index in iif_amd/cifar.py OPS) and its constants, built as cifar.policy_table builds
// them at h = w = S.
//
// One 1024-thread block per image; thread t owns the output pixels p = t, t + 1024, ... (row p / S, column p % S).  An fp32
// image at S = 224 is 602 KB, more than LDS holds, so the block works in SWEEPS over its image and keeps the pixels in
// global memory between them, ping-ponging between `out` and the caller's `work` buffer (the last sweep writes `out`):
//   - pointwise ops (Color, Posterize, Solarize, Brightness, Invert) run inside whichever sweep is running;
//   - an op that needs a whole-image reduction (Contrast's grey mean, AutoContrast's channel min / max, Equalize's
//     histograms) has its data accumulated by the sweep before it and applies at the start of the next sweep;
//   - a gather (the five affine ops, Sharpness' 3x3 neighbours) starts a sweep that reads the previous sweep's buffer.
// So a record with k reduction / gather ops takes k + 1 sweeps (at most 3), Normalize folded into the last one.
// Hand-off between sweeps: the pixels one thread wrote are read by other threads of the same block.  Every thread drains
// its stores (s_waitcnt vmcnt(0)) before the block barrier, and every read of a buffer written by an earlier sweep is an
// agent-scope relaxed atomic load, which bypasses the CU's L1 (global_load ... sc1), so no stale L1 line can be read.
// No block reads another block's image.
//
// Arithmetic: each op is augment.apply_op_signed's torch expression in fp32, operation by operation (-ffp-contract=off,
// IEEE division), as cifar_augment.hip computes it; Contrast's grey mean sums in double, Sharpness' 3x3 blur in another order
// than conv2d.  A malformed descriptor or an unknown op code gives a zero image.
#include "lt_resample.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / IIF_WAVE;
constexpr int kSlots = 2, kRecWords = 8;      // op records per image, words per record

// op codes = the index in iif_amd/cifar.py OPS
enum { OP_SHEARX, OP_SHEARY, OP_TRANSLATEX, OP_TRANSLATEY, OP_ROTATE, OP_COLOR, OP_POSTERIZE, OP_SOLARIZE, OP_CONTRAST,
       OP_SHARPNESS, OP_BRIGHTNESS, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT, OP_COUNT };
enum Kind { K_POINT, K_REDUCE, K_GATHER };

__device__ __forceinline__ Kind kind(int op) {
    if (op <= OP_ROTATE || op == OP_SHARPNESS) return K_GATHER;
    if (op == OP_CONTRAST || op == OP_AUTOCONTRAST || op == OP_EQUALIZE) return K_REDUCE;
    return K_POINT;
}

struct Op {
    int code;
    uint32_t iw;                                        // posterize mask / solarize threshold
    float k[6];                                         // affine a .. f, or blend (f, 1 - f)
};

struct PolicyArgs {
    const unsigned char* pool; int64_t pool_bytes;
    const int64_t* desc; const uint32_t* ops;
    float* work; float* out; int S;
    float mean[3], stdv[3];
};

struct Lds {
    int hist[3][256];
    int lut[3][256];
    int last[3];
    int wtot[3][4];
    double dred[kWaves];
    float fred[kWaves][6];
    float stat[6];                                      // grey mean, or lo[3] / hi[3]
};

// lt_augment_kernel's descriptor check: a descriptor outside the pool or the resized image reads nothing
__device__ __forceinline__ bool desc_ok(const int64_t* d, int64_t pool_bytes, int S) {
    const int64_t off = d[D_OFF], h = d[D_H], w = d[D_W], rh = d[D_RH], rw = d[D_RW], oy = d[D_OY], ox = d[D_OX];
    return off >= 0 && h > 0 && w > 0 && h <= INT32_MAX && w <= INT32_MAX && w <= pool_bytes && h <= pool_bytes / (3 * w) &&
           off <= pool_bytes - 3 * h * w && rh > 0 && rw > 0 && rh <= INT32_MAX && rw <= INT32_MAX && oy >= 0 && ox >= 0 &&
           oy + S <= rh && ox + S <= rw;
}

__device__ __forceinline__ int to_u8(float v) { return (int)fminf(fmaxf(rintf(v * 255.0f), 0.0f), 255.0f); }

// a pixel written by another thread in an earlier sweep: an L1-bypassing load (global_load_dword ... sc1)
__device__ __forceinline__ float load_l2(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every thread's stores leave the CU before the barrier that ends a sweep
__device__ __forceinline__ void end_sweep() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

__device__ __forceinline__ void pointwise(float (&v)[3], const Op& o) {
    switch (o.code) {
    case OP_COLOR: {                                    // adjust_saturation: blend with the grey image
        const float g = grey(v);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = blend(v[c], g, o.k[0], o.k[1]);
        break;
    }
    case OP_BRIGHTNESS:                                 // adjust_brightness: blend with 0
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = blend(v[c], 0.0f, o.k[0], o.k[1]);
        break;
    case OP_POSTERIZE:
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)(to_u8(v[c]) & (int)o.iw) / 255.0f;
        break;
    case OP_SOLARIZE:
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int u = to_u8(v[c]);
            v[c] = (float)(u < (int)o.iw ? u : 255 - u) / 255.0f;
        }
        break;
    case OP_INVERT:
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = 1.0f - v[c];
        break;
    default:
        break;
    }
}

// a reduction op on one pixel, with the statistics of the image it reads (Lds::stat, Lds::lut)
__device__ __forceinline__ void reduce_apply(float (&v)[3], const Op& o, const Lds& s) {
    if (o.code == OP_CONTRAST) {                        // adjust_contrast: blend with the grey image's mean
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = blend(v[c], s.stat[0], o.k[0], o.k[1]);
    } else if (o.code == OP_AUTOCONTRAST) {             // augment._autocontrast
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float l = s.stat[c], h = s.stat[3 + c];
            if (h > l) v[c] = (v[c] - l) * (1.0f / fmaxf(h - l, 1e-12f));
        }
    } else {                                            // augment._equalize (the LUT keeps a channel whose step is 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)s.lut[c][to_u8(v[c])] / 255.0f;
    }
}

// a gather op at pixel (y, x) from the previous sweep's image `cur`
__device__ __forceinline__ void gather(float (&v)[3], const Op& o, const float* cur, int S, int y, int x) {
    const int npix = S * S;
    if (o.code == OP_SHARPNESS) {                       // augment._sharpness: the (1 1 1; 1 5 1; 1 1 1) / 13 blur, borders kept
        const int p = y * S + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = load_l2(cur + c * npix + p);
        const bool inner = y >= 1 && y <= S - 2 && x >= 1 && x <= S - 2;
        const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float blur = v[c];
            if (inner) {
                const float* q = cur + c * npix + p;
                float acc = 0.0f;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) acc += ((dy | dx) ? k1 : k5) * load_l2(q + dy * S + dx);
                blur = acc;
            }
            v[c] = blend(v[c], blur, o.k[0], o.k[1]);
        }
        return;
    }
    // PIL AFFINE as augment._affine: output (x, y) reads input floor(((a xs) + (b ys)) + c), floor(((d xs) + (e ys)) + f)
    // at pixel centres xs = x + 0.5, ys = y + 0.5; grey 128 / 255 outside
    const float xs = (float)x + 0.5f, ys = (float)y + 0.5f;
    const float fx = floorf((o.k[0] * xs + o.k[1] * ys) + o.k[2]);
    const float fy = floorf((o.k[3] * xs + o.k[4] * ys) + o.k[5]);
    const bool in = fx >= 0.0f && fx < (float)S && fy >= 0.0f && fy < (float)S;
    const int p = in ? (int)fy * S + (int)fx : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = in ? load_l2(cur + c * npix + p) : 128.0f / 255.0f;
}

// the statistics a reduction op needs, accumulated per thread over its pixels
struct Acc {
    double gsum;
    float lo[3], hi[3];
};

__device__ __forceinline__ void accumulate(Acc& a, const float (&v)[3], int op, Lds& s) {
    if (op == OP_CONTRAST) {
        a.gsum += (double)grey(v);
    } else if (op == OP_AUTOCONTRAST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a.lo[c] = fminf(a.lo[c], v[c]);
            a.hi[c] = fmaxf(a.hi[c], v[c]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) atomicAdd(&s.hist[c][to_u8(v[c])], 1);
    }
}

// block-wide combination of the accumulated statistics into Lds::stat / Lds::lut; called by every thread after end_sweep()
__device__ void finish_stats(Acc& a, int op, Lds& s, int npix) {
    const int t = threadIdx.x, lane = t & (IIF_WAVE - 1), w = t / IIF_WAVE;
    if (op == OP_CONTRAST) {
        double v = a.gsum;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) s.dred[w] = v;
        __syncthreads();
        if (t == 0) {
            double tot = 0.0;
            for (int i = 0; i < kWaves; ++i) tot += s.dred[i];
            s.stat[0] = (float)(tot / (double)npix);
        }
    } else if (op == OP_AUTOCONTRAST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float l = -wave_max(-a.lo[c]), h = wave_max(a.hi[c]);
            if (lane == 0) { s.fred[w][c] = l; s.fred[w][3 + c] = h; }
        }
        __syncthreads();
        if (t < 6) {
            float r = s.fred[0][t];
            for (int i = 1; i < kWaves; ++i) r = t < 3 ? fminf(r, s.fred[i][t]) : fmaxf(r, s.fred[i][t]);
            s.stat[t] = r;
        }
    } else {
        // PIL.ImageOps.equalize per channel: lut[i] = (#pixels below i + step / 2) / step, step = (pixels - count of the
        // last non-empty bin) / 255; step 0 keeps the channel.  Thread t < 768 owns bin t & 255 of channel t >> 8.
        const int c = t >> 8, i = t & 255, cw = (t >> 6) & 3;
        int h = 0, inc = 0;
        if (t < 768) {
            h = s.hist[c][i];
            if (h > 0) atomicMax(&s.last[c], i);
            inc = h;
#pragma unroll
            for (int o = 1; o < IIF_WAVE; o <<= 1) {
                const int q = __shfl_up(inc, o, IIF_WAVE);
                if (lane >= o) inc += q;
            }
            if (lane == IIF_WAVE - 1) s.wtot[c][cw] = inc;
        }
        __syncthreads();
        if (t < 768) {
            int below = inc - h;
            for (int k = 0; k < cw; ++k) below += s.wtot[c][k];
            const int step = (npix - s.hist[c][s.last[c]]) / 255;
            s.lut[c][i] = step > 0 ? min((below + step / 2) / step, 255) : i;
        }
        __syncthreads();
        if (t < 768) s.hist[c][i] = 0;                 // ready for a second Equalize
        if (t < 3) s.last[t] = 0;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kThreads) lt_policy_kernel(PolicyArgs a) {
    __shared__ Lds s;
    const int b = blockIdx.x, t = threadIdx.x;
    const int S = a.S, npix = S * S;
    const int64_t img = (int64_t)b * 3 * npix;
    const int64_t* d = a.desc + (int64_t)b * D_WORDS;

    // the applied ops of the record, in order (two named registers: a dynamically indexed array would go to LDS)
    Op op0{}, op1{};
    int n = 0;
    bool ok = desc_ok(d, a.pool_bytes, S);
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
        const uint32_t* r = a.ops + ((int64_t)b * kSlots + j) * kRecWords;
        const uint32_t code = r[0];
        if (code == IIF_LT_OP_NONE) continue;
        if (code >= OP_COUNT) ok = false;
        Op o;
        o.code = (int)code;
        o.iw = r[1];
#pragma unroll
        for (int i = 0; i < 6; ++i) o.k[i] = __uint_as_float(r[1 + i]);
        if (n == 0) op0 = o; else op1 = o;
        ++n;
    }
    if (!ok) {                                          // reads nothing: a zero image
        for (int p = t; p < 3 * npix; p += kThreads) a.out[img + p] = 0.0f;
        return;
    }

    if (t < 768) s.hist[t >> 8][t & 255] = 0;
    if (t < 3) s.last[t] = 0;
    __syncthreads();

    int nsweeps = 1;
    nsweeps += (n > 0 && kind(op0.code) != K_POINT) + (n > 1 && kind(op1.code) != K_POINT);
    const unsigned char* src = a.pool + d[D_OFF];
    const int h = (int)d[D_H], w = (int)d[D_W], oy = (int)d[D_OY], ox = (int)d[D_OX];
    const bool flip = d[D_FLIP] != 0;
    const float sy = (float)h / (float)d[D_RH], sx = (float)w / (float)d[D_RW];   // area_pixel_compute_scale: in / out in fp32

    const float* cur = nullptr;
    int j0 = 0;                                         // first op of this sweep (sweeps after the first start with a non-pointwise op)
    for (int sweep = 0; sweep < nsweeps; ++sweep) {
        float* dst = (((nsweeps - 1 - sweep) & 1) ? a.work : a.out) + img;
        // the ops of this sweep: j0 (if it is a reduction / gather, only after the first sweep), then pointwise ops up to
        // the next non-pointwise op `j1`, whose statistics this sweep accumulates if it is a reduction
        int j1 = sweep == 0 ? 0 : j0 + 1;
        while (j1 < n && kind((j1 ? op1 : op0).code) == K_POINT) ++j1;
        const bool last = j1 >= n;
        const Op& first = j0 ? op1 : op0;
        const Kind first_kind = sweep == 0 ? K_POINT : kind(first.code);
        const int next_op = last ? -1 : (j1 ? op1 : op0).code;
        const bool acc_stats = !last && kind(next_op) == K_REDUCE;
        Acc acc;
        acc.gsum = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { acc.lo[c] = INFINITY; acc.hi[c] = -INFINITY; }

        for (int p = t; p < npix; p += kThreads) {
            const int y = p / S, x = p - y * S;
            float v[3];
            int j = j0;
            if (sweep == 0) {
                resample(src, h, w, sy, sx, oy + y, ox + (flip ? S - 1 - x : x), v);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = clamp01(v[c]);
            } else if (first_kind == K_GATHER) {
                gather(v, first, cur, S, y, x);
                ++j;
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = load_l2(cur + c * npix + p);
                reduce_apply(v, first, s);
                ++j;
            }
            for (; j < j1; ++j) pointwise(v, j ? op1 : op0);
            if (acc_stats) accumulate(acc, v, next_op, s);
            if (last) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[c * npix + p] = (v[c] - a.mean[c]) / a.stdv[c];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[c * npix + p] = v[c];
            }
        }
        if (last) break;
        end_sweep();
        if (acc_stats) finish_stats(acc, next_op, s, npix);
        cur = dst;
        j0 = j1;
    }
}

}  // namespace

extern "C" int iif_lt_augment_policy(const uint8_t* pool, int64_t pool_bytes, const int64_t* desc, const uint32_t* ops,
                                     int64_t batch, int size, const float* mean_std, float* work, float* out, void* stream) {
    if (!pool || !desc || !ops || !mean_std || !work || !out) return IIF_EINVAL;
    if (pool_bytes < 0 || batch < 0 || batch > INT32_MAX || size <= 0 || size > 16384) return IIF_EINVAL;
    if (batch == 0) return IIF_OK;
    PolicyArgs a{pool, pool_bytes, desc, ops, work, out, size, {}, {}};
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = mean_std[c];
        a.stdv[c] = mean_std[3 + c];
    }
    hipLaunchKernelGGL(lt_policy_kernel, dim3((unsigned)batch), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}
