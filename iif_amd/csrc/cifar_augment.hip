// CIFAR training input for gfx950 (MI355X): one launch builds a whole augmented batch from the device-resident uint8
// dataset, in the order of the reference's load_cifar (classification/initialisers.py:116-134) -
//   pad 4 with 0 -> random 32x32 crop -> horizontal flip (p 0.5)          [IIF_CIFAR_CROP_FLIP]
//   -> x / 255 -> one CIFAR10Policy sub-policy (iif_amd/augment.py)        [IIF_CIFAR_POLICY]
//   -> Cutout(1, 16), pixels zeroed                                         [IIF_CIFAR_CUTOUT]
//   -> (x - mean) / std with the reference's CIFAR mean / std.
//
// One 256-thread block per image.  Thread t owns row t >> 3, columns 4 (t & 7) .. +3 of all three channels (12 values in
// registers) and stores them as three float4.  Gathers (the affine ops, Sharpness' 3x3 neighbours) go through one 12 KB
// LDS copy of the image; the reductions (AutoContrast's min / max, Contrast's grey mean) are wave shuffles plus four LDS
// slots; Equalize builds 256-bin LDS histograms with integer atomics and a wave-scan prefix sum.
//
// Randomness: draw slot s of the image at position `pos` of this rank's epoch list is the upper 32 bits of
//   mix(mix(mix(mix(mix(seed) ^ epoch) ^ rank) ^ pos) ^ s),   mix = the splitmix64 finaliser (add the golden gamma, then
// xor-shift-multiply twice, xor-shift); iif_amd/cifar.py restates it in numpy.  Integer draws in [0, n) take
// (u * n) >> 32; a probability p applies when (u >> 8) < round(p * 2^24); flip and sign take the top bit.
//
// Arithmetic: each op is augment.py's torch expression in fp32, operation by operation (-ffp-contract=off, IEEE
// division), with its per-(sub-policy, op, sign) constants precomputed on the host from augment.py's own tables.  The
// two sums (Contrast's grey mean, Sharpness' 3x3 blur) add in another order than torch does.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSide = 32, kPix = kSide * kSide;
constexpr unsigned kAllFlags = IIF_CIFAR_CROP_FLIP | IIF_CIFAR_POLICY | IIF_CIFAR_CUTOUT;

// op codes = the index in iif_amd/cifar.py OPS
enum { OP_SHEARX, OP_SHEARY, OP_TRANSLATEX, OP_TRANSLATEY, OP_ROTATE, OP_COLOR, OP_POSTERIZE, OP_SOLARIZE, OP_CONTRAST,
       OP_SHARPNESS, OP_BRIGHTNESS, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT };

// param slots (also the draw slots)
enum { P_CROP_Y, P_CROP_X, P_FLIP, P_SUB, P_APPLY0, P_SIGN0, P_APPLY1, P_SIGN1, P_CUT_Y, P_CUT_X };

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned draw(uint64_t key, unsigned slot) { return (unsigned)(mix64(key ^ slot) >> 32); }
__device__ __forceinline__ int below(unsigned u, unsigned n) { return (int)(((uint64_t)u * n) >> 32); }

struct Lds {
    float img[3 * kPix];
    int hist[3][256];
    int lut[3][256];
    int last[3];
    int wtot[3][kThreads / IIF_WAVE];
    float red[kThreads / IIF_WAVE][6];
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ int to_u8(float v) { return (int)fminf(fmaxf(rintf(v * 255.0f), 0.0f), 255.0f); }

__device__ __forceinline__ void to_lds(Lds& s, const float (&v)[3][4], int p0) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) s.img[c * kPix + p0 + j] = v[c][j];
}

// PIL AFFINE as augment._affine: output (x, y) reads input floor(((a xs) + (b ys)) + c), floor(((d xs) + (e ys)) + f) at
// pixel centres xs = x + 0.5, ys = y + 0.5; grey 128 / 255 outside
__device__ void op_affine(Lds& s, float (&v)[3][4], int y, int x0, const float* k) {
    to_lds(s, v, y * kSide + x0);
    __syncthreads();
    const float fill = 128.0f / 255.0f;
    const float ys = (float)y + 0.5f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float xs = (float)(x0 + j) + 0.5f;
        const int sx = (int)floorf((k[0] * xs + k[1] * ys) + k[2]);
        const int sy = (int)floorf((k[3] * xs + k[4] * ys) + k[5]);
        const bool ok = sx >= 0 && sx < kSide && sy >= 0 && sy < kSide;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][j] = ok ? s.img[c * kPix + sy * kSide + sx] : fill;
    }
    __syncthreads();
}

// _blend: clamp(F x + G o, 0, 1) with F = f, G = 1 - f rounded from double on the host
__device__ __forceinline__ float blend(float x, float o, float F, float G) { return clamp01(F * x + G * o); }

__device__ __forceinline__ float grey(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }

// sum over the block, the same value in every thread (fixed order: waves 0..3)
__device__ float block_sum(Lds& s, float v) {
    v = wave_sum(v);
    const int w = threadIdx.x / IIF_WAVE;
    if ((threadIdx.x & (IIF_WAVE - 1)) == 0) s.red[w][0] = v;
    __syncthreads();
    const float t = (s.red[0][0] + s.red[1][0]) + (s.red[2][0] + s.red[3][0]);
    __syncthreads();
    return t;
}

__device__ void op_autocontrast(Lds& s, float (&v)[3][4]) {
    float lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = fminf(fminf(v[c][0], v[c][1]), fminf(v[c][2], v[c][3]));
        hi[c] = fmaxf(fmaxf(v[c][0], v[c][1]), fmaxf(v[c][2], v[c][3]));
        lo[c] = -wave_max(-lo[c]);
        hi[c] = wave_max(hi[c]);
    }
    const int w = threadIdx.x / IIF_WAVE;
    if ((threadIdx.x & (IIF_WAVE - 1)) == 0)
        for (int c = 0; c < 3; ++c) { s.red[w][c] = lo[c]; s.red[w][3 + c] = hi[c]; }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float l = fminf(fminf(s.red[0][c], s.red[1][c]), fminf(s.red[2][c], s.red[3][c]));
        const float h = fmaxf(fmaxf(s.red[0][3 + c], s.red[1][3 + c]), fmaxf(s.red[2][3 + c], s.red[3][3 + c]));
        if (h > l) {
            const float scale = 1.0f / fmaxf(h - l, 1e-12f);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = (v[c][j] - l) * scale;
        }
    }
    __syncthreads();
}

// PIL.ImageOps.equalize per channel (augment._equalize): lut[i] = (#pixels below i + step / 2) / step,
// step = (pixels - count of the last non-empty bin) / 255; step 0 keeps the (quantised) channel
__device__ void op_equalize(Lds& s, float (&v)[3][4]) {
    const int t = threadIdx.x, lane = t & (IIF_WAVE - 1), w = t / IIF_WAVE;
    int u[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.hist[c][t] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) u[c][j] = to_u8(v[c][j]);
    }
    if (t < 3) s.last[t] = 0;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(&s.hist[c][u[c][j]], 1);
    __syncthreads();
    int h[3], inc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        h[c] = s.hist[c][t];
        if (h[c] > 0) atomicMax(&s.last[c], t);
        inc[c] = h[c];
#pragma unroll
        for (int o = 1; o < IIF_WAVE; o <<= 1) {
            const int q = __shfl_up(inc[c], o, IIF_WAVE);
            if (lane >= o) inc[c] += q;
        }
        if (lane == IIF_WAVE - 1) s.wtot[c][w] = inc[c];
    }
    __syncthreads();
    int step[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int below_w = 0;
        for (int k = 0; k < w; ++k) below_w += s.wtot[c][k];
        step[c] = (kPix - s.hist[c][s.last[c]]) / 255;
        if (step[c] > 0) s.lut[c][t] = min((below_w + inc[c] - h[c] + step[c] / 2) / step[c], 255);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[c][j] = (float)(step[c] > 0 ? s.lut[c][u[c][j]] : u[c][j]) / 255.0f;
    __syncthreads();
}

// PIL.ImageEnhance.Sharpness as augment._sharpness: blend with the (1 1 1; 1 5 1; 1 1 1) / 13 smoothing, borders kept
__device__ void op_sharpness(Lds& s, float (&v)[3][4], int y, int x0, float F, float G) {
    to_lds(s, v, y * kSide + x0);
    __syncthreads();
    const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        if (y < 1 || y > kSide - 2 || x < 1 || x > kSide - 2) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* p = s.img + c * kPix + y * kSide + x;
            float acc = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) acc += ((dy | dx) ? k1 : k5) * p[dy * kSide + dx];
            v[c][j] = blend(v[c][j], acc, F, G);
        }
    }
    __syncthreads();
}

// one operation of a sub-policy; k = its 8-word entry of the constant table: [op, threshold, p0 .. p5]
__device__ void apply_op(Lds& s, float (&v)[3][4], int y, int x0, const unsigned* k) {
    const int op = (int)k[0];
    float kf[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) kf[i] = __uint_as_float(k[2 + i]);
    const float F = kf[0], G = kf[1];
    switch (op) {
    case OP_SHEARX: case OP_SHEARY: case OP_TRANSLATEX: case OP_TRANSLATEY: case OP_ROTATE:
        op_affine(s, v, y, x0, kf);
        break;
    case OP_COLOR:                                      // adjust_saturation: blend with the grey image
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float g = grey(v[0][j], v[1][j], v[2][j]);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = blend(v[c][j], g, F, G);
        }
        break;
    case OP_CONTRAST: {                                 // adjust_contrast: blend with the grey image's mean
        float part = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) part += grey(v[0][j], v[1][j], v[2][j]);
        const float mean = block_sum(s, part) / (float)kPix;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = blend(v[c][j], mean, F, G);
        break;
    }
    case OP_BRIGHTNESS:                                 // adjust_brightness: blend with 0
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = blend(v[c][j], 0.0f, F, G);
        break;
    case OP_SHARPNESS:
        op_sharpness(s, v, y, x0, F, G);
        break;
    case OP_POSTERIZE: {
        const int mask = (int)k[2];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = (float)(to_u8(v[c][j]) & mask) / 255.0f;
        break;
    }
    case OP_SOLARIZE: {
        const int thr = (int)k[2];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int u = to_u8(v[c][j]);
                v[c][j] = (float)(u < thr ? u : 255 - u) / 255.0f;
            }
        break;
    }
    case OP_AUTOCONTRAST:
        op_autocontrast(s, v);
        break;
    case OP_EQUALIZE:
        op_equalize(s, v);
        break;
    case OP_INVERT:
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = 1.0f - v[c][j];
        break;
    default:
        break;
    }
}

struct AugArgs {
    const unsigned char* data; int64_t n;
    const int64_t* labels; const int64_t* index;
    int64_t pos0; uint64_t seed; int64_t epoch, rank;
    unsigned flags; const unsigned* policy;
    float* out; int64_t* targets; int32_t* params;
};

__global__ __launch_bounds__(kThreads) void cifar_augment_kernel(AugArgs a) {
    __shared__ Lds s;
    const int b = blockIdx.x, t = threadIdx.x;
    const int y = t >> 3, x0 = (t & 7) * 4;

    const uint64_t key = mix64(mix64(mix64(mix64(a.seed) ^ (uint64_t)a.epoch) ^ (uint64_t)a.rank) ^ (uint64_t)(a.pos0 + b));
    int prm[10];
    prm[P_CROP_Y] = below(draw(key, P_CROP_Y), 9);
    prm[P_CROP_X] = below(draw(key, P_CROP_X), 9);
    prm[P_FLIP] = (int)(draw(key, P_FLIP) >> 31);
    prm[P_SUB] = below(draw(key, P_SUB), 25);
    prm[P_CUT_Y] = below(draw(key, P_CUT_Y), kSide);
    prm[P_CUT_X] = below(draw(key, P_CUT_X), kSide);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        // the application threshold lives in the table (both sign entries carry it); without POLICY there is no table
        const unsigned u = draw(key, P_APPLY0 + 2 * j);
        const unsigned thr = (a.flags & IIF_CIFAR_POLICY) ? a.policy[((prm[P_SUB] * 2 + j) * 2) * 8 + 1] : 0u;
        prm[P_APPLY0 + 2 * j] = (u >> 8) < thr;
        prm[P_SIGN0 + 2 * j] = 1 - (int)(draw(key, P_SIGN0 + 2 * j) >> 31);   // 1: positive
    }
    if (a.params && t == 0)
#pragma unroll
        for (int i = 0; i < 10; ++i) a.params[(int64_t)b * 10 + i] = prm[i];

    float* out = a.out + (int64_t)b * 3 * kPix;
    const int64_t src = a.index[b];
    if (src < 0 || src >= a.n) {                      // reads nothing: a zero image and label -1 (check_labels raises)
        if (t == 0) a.targets[b] = -1;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<f32x4*>(out + c * kPix + y * kSide + x0) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }
    if (t == 0) a.targets[b] = a.labels[src];

    // pad 4 + crop + flip, then ToTensor's x / 255
    const unsigned char* img = a.data + src * (3 * kPix);
    const bool cf = a.flags & IIF_CIFAR_CROP_FLIP;
    const int sy = cf ? y + prm[P_CROP_Y] - 4 : y;
    float v[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        const int sx = cf ? (prm[P_FLIP] ? kSide - 1 - x : x) + prm[P_CROP_X] - 4 : x;
        const bool in = sy >= 0 && sy < kSide && sx >= 0 && sx < kSide;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][j] = in ? (float)img[c * kPix + sy * kSide + sx] / 255.0f : 0.0f;
    }

    if (a.flags & IIF_CIFAR_POLICY) {
        const unsigned* e0 = a.policy + ((prm[P_SUB] * 2 + 0) * 2 + prm[P_SIGN0]) * 8;
        const unsigned* e1 = a.policy + ((prm[P_SUB] * 2 + 1) * 2 + prm[P_SIGN1]) * 8;
#pragma unroll 1
        for (int j = 0; j < 2; ++j)
            if (j ? prm[P_APPLY1] : prm[P_APPLY0]) apply_op(s, v, y, x0, j ? e1 : e0);
    }

    if (a.flags & IIF_CIFAR_CUTOUT) {
        const int cy = prm[P_CUT_Y], cx = prm[P_CUT_X];
        if (y >= cy - 8 && y < cy + 8)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j >= cx - 8 && x0 + j < cx + 8) v[0][j] = v[1][j] = v[2][j] = 0.0f;
    }

    const float mean[3] = {0.4914f, 0.4822f, 0.4465f}, stdv[3] = {0.2023f, 0.1994f, 0.2010f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (v[c][j] - mean[c]) / stdv[c];
        *reinterpret_cast<f32x4*>(out + c * kPix + y * kSide + x0) = o;
    }
}

}  // namespace

extern "C" int iif_cifar_augment(const uint8_t* data, int64_t n, const int64_t* labels, const int64_t* index, int64_t batch,
                                 int64_t pos0, uint64_t seed, int64_t epoch, int64_t rank, uint32_t flags,
                                 const uint32_t* policy, float* out, int64_t* targets, int32_t* params, void* stream) {
    if (!data || !labels || !index || !out || !targets) return IIF_EINVAL;
    if (n <= 0 || batch < 0 || batch > INT32_MAX || pos0 < 0 || (flags & ~kAllFlags)) return IIF_EINVAL;
    if ((flags & IIF_CIFAR_POLICY) && !policy) return IIF_EINVAL;
    if (batch == 0) return IIF_OK;
    AugArgs a{data, n, labels, index, pos0, seed, epoch, rank, flags, policy, out, targets, params};
    hipLaunchKernelGGL(cifar_augment_kernel, dim3((unsigned)batch), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}
