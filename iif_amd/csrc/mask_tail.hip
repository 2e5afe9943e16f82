// The tail of the Mask R-CNN head fused, gfx950: the 2x2 / stride-2 deconvolution, its ReLU and the class-selected predictor.
//
// Reference: FCNMaskHead.forward ends with x = relu(upsample(x)); mask_pred = conv_logits(x) (fcn_mask_head.py:131-136).  A
// ConvTranspose2d with kernel = stride = 2 is a plain GEMM: up_weight [Ci][Co][2][2] read as B [Ci][4 Co] (column j = 4 co + ab,
// ab = 2 a + b) maps the Ci vector of input pixel p = (i, j) to the four output pixels P = (2i + a, 2j + b) below it.  With
// l = labels[n]:
//   pre[n, p, j] = up_bias[co] + sum_ci f[n, ci, p] B[ci, j]         y = max(pre, 0)
//   z[n, P]      = bias[l] + sum_co weight[l, co] y[n, p, 4 co + ab]
// The [N, Co, 2h, 2w] activation y and its gradient are never stored.  Four matmul-shaped kernels on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32, bit for bit a k-ordered fmaf chain), all float32 with bfloat16 f widened exactly:
//   forward   block (64 pixels, RoI): GEMM over Ci per group of 256 columns, epilogue + up_bias, ReLU, times the selected
//             weight row, summed over co in registers; then the bias, the BCE rows and the compact gradient g0 [N][4hw]
//   rows      the backward's recomputation of the same GEMM, block (column group, RoI): the sign of pre as one bit per
//             (RoI, pixel, column) and the per-RoI rows sum_P g y [N][Co + 1] of dweight / dbias
//   df        block (64 pixels, RoI): [Ci][4 Co] x [4 Co][pixels], the second operand generated on the fly as
//             g * weight[l, co] * sign; every element of df written once
//   dup       block (64 ci, 128 columns, RoI range): [Ci][pixels] x [pixels][4 Co] with the same generated operand, one partial
//             per RoI range, summed in range order; dup_bias from the column sums of the generated operand
// dweight / dbias: the per-class segment sum of mask_predict_core.h on the rows.  No float atomics: the same bits from call to call.
// The iif_mask_tail_loss_* entries leave the divisor to the device: g = sigmoid(z) - t is stored undivided,
// mask_predict_finish_kernel counts the valid rows and writes *inv_div, and rows / df / dup multiply by u = up * inv_div; in
// their forward, rows and df grids block y takes the y-th valid RoI (valid_first_roi), so the blocks with work come first.
#include "common.h"
#include "loss_reduce.h"
#include "mask_predict_core.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int kMaxC = 1024, kMaxInHW = 1024; // Ci, Co; input pixels per RoI
constexpr int kPix = 64;                     // pixels per block: two 32-row MFMA tiles
static_assert(kPix >= kMinTile, "the wrappers allocate one row partial per kMinTile pixels");
constexpr int kCols = 128;                   // columns per chunk: one 32-column MFMA tile per wave; forward / rows: two chunks
constexpr int kSlab = 32;                    // Ci values staged per round

__device__ __forceinline__ int crow(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }   // C/D row of register r
// the output pixel (2i + a, 2j + b) of input pixel p = i * w + j in a [2h][2w] map
__device__ __forceinline__ int out_pixel(int p, int ab, int w) {
    const int i = p / w, j = p - i * w;
    return (2 * i + (ab >> 1)) * (2 * w) + 2 * j + (ab & 1);
}

// One slab of f for the block, kSlab x 64 values, kSlab / 4 per thread: thread (px = tid & 63, row0 = tid >> 6) holds rows row0 + 4 rr.
template <typename T>
__device__ __forceinline__ void load_slab(const T* __restrict__ fn, int ci, int hw, int p0, int k0, float (&stg)[kSlab / 4]) {
    const int px = threadIdx.x & 63, row0 = threadIdx.x >> 6;
    const bool pok = p0 + px < hw;
#pragma unroll
    for (int rr = 0; rr < kSlab / 4; ++rr) {
        const int k = k0 + rr * 4 + row0;
        stg[rr] = (pok && k < ci) ? VT<T>::load1(fn + (int64_t)k * hw + p0 + px) : 0.f;
    }
}

// acc[c][s][.] = sum_ci f[n, ci, p0 + 32 s + row] * B[ci, j + 128 c]: rows on the registers, the column on the lane (both lane
// halves); c < ncl.  Per round of kSlab values of ci the wave first asks for its own B values (they arrive while the block
// stages f), the block writes the slab of f it holds in registers (`stg`, loaded one round ahead) to LDS - row k swizzled by 32
// columns where k is odd, so the two lane halves, which read rows k and k + 1, fall on different banks - and asks for the next
// slab; after the last round that is the first slab of the tile at p0_next, which the next call finds in `stg`.
template <typename T>
__device__ __forceinline__ void tail_gemm(const T* __restrict__ fn, const float* __restrict__ upw, int ci, int ld, int hw, int p0,
                                          int p0_next, int nsub, int j, int ncl, float* sA, float (&stg)[kSlab / 4],
                                          f32x16 (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, li = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][0][r] = 0.f; acc[0][1][r] = 0.f; acc[1][0][r] = 0.f; acc[1][1][r] = 0.f; }
    for (int k0 = 0; k0 < ci; k0 += kSlab) {
        float b[2][kSlab / 2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int s = 0; s < kSlab / 2; ++s) {
                const int k = k0 + 2 * s + half, jc = j + c * kCols;
                b[c][s] = (jc < ld && k < ci) ? upw[(int64_t)k * ld + jc] : 0.f;
            }
        __syncthreads();                                 // the previous round's (or call's) reads of sA are done
        {
            const int px = tid & 63, row0 = tid >> 6;
#pragma unroll
            for (int rr = 0; rr < kSlab / 4; ++rr) {
                const int row = rr * 4 + row0;
                sA[row * 64 + (px ^ ((row & 1) << 5))] = stg[rr];
            }
        }
        __syncthreads();
        const bool last = k0 + kSlab >= ci;
        load_slab<T>(fn, ci, hw, last ? p0_next : p0, last ? 0 : k0 + kSlab, stg);
#pragma unroll
        for (int sc = 0; sc < kSlab / 16; ++sc) {
            if (k0 + 16 * sc >= ci) break;
#pragma unroll
            for (int s = 8 * sc; s < 8 * sc + 8; ++s) {
                const float* ar = sA + (2 * s + half) * 64;
                const float a0 = ar[li ^ (half << 5)], a1 = ar[(32 + li) ^ (half << 5)];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[0][s], acc[0][0], 0, 0, 0);
                if (nsub > 1) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[0][s], acc[0][1], 0, 0, 0);
                if (ncl > 1) {
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[1][s], acc[1][0], 0, 0, 0);
                    if (nsub > 1) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[1][s], acc[1][1], 0, 0, 0);
                }
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256, 2) mask_tail_fwd_kernel(const T* __restrict__ f, const float* __restrict__ upw,
                                                            const float* __restrict__ upb, const float* __restrict__ weight,
                                                            int64_t ld_w, const float* __restrict__ bias,
                                                            const int64_t* __restrict__ labels, const float* __restrict__ target,
                                                            int C, int ci, int co, int w, int hw, float inv, int valid_first,
                                                            float* __restrict__ z, float* __restrict__ g0,
                                                            float* __restrict__ row_loss, int* status) {
    __shared__ float sA[kSlab * 64];
    __shared__ float zs[4][kPix][4];
    __shared__ float wl[4];
    __shared__ int slot[5];
    const int n = valid_first ? valid_first_roi(labels, gridDim.y, C, blockIdx.y, slot) : blockIdx.y;
    const int p0 = blockIdx.x * kPix, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int64_t lb = labels[n];
    const int opx = tid >> 2, oab = tid & 3;             // the output this thread finishes
    const bool live = p0 + opx < hw;
    const int64_t o = live ? (int64_t)n * 4 * hw + out_pixel(p0 + opx, oab, w) : 0;
    if (lb < 0 || lb >= C) {                             // block-uniform
        if (tid == 0) {
            if (status) atomicOr(status, 1);
            if (row_loss) row_loss[(int64_t)n * gridDim.x + blockIdx.x] = 0.f;
        }
        if (live) {
            if (z) z[o] = 0.f;
            if (g0) g0[o] = 0.f;
        }
        return;
    }
    const float* wrow = weight + lb * ld_w;
    const int ld = 4 * co, nsub = min(2, (hw - p0 + 31) / 32);
    const T* fn = f + (int64_t)n * ci * hw;
    float zacc[2][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { zacc[0][r] = 0.f; zacc[1][r] = 0.f; }
    float stg[kSlab / 4];
    load_slab<T>(fn, ci, hw, p0, 0, stg);
    for (int j0 = 0; j0 < ld; j0 += 2 * kCols) {
        const int j = j0 + wave * 32 + (lane & 31), ncl = j0 + kCols < ld ? 2 : 1;
        f32x16 acc[2][2];
        tail_gemm<T>(fn, upw, ci, ld, hw, p0, p0, nsub, j, ncl, sA, stg, acc);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int cidx = (j + c * kCols) >> 2;
            const bool ok = cidx < co;
            const float ub = (ok && upb) ? upb[cidx] : 0.f, wv = ok ? wrow[cidx] : 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r) zacc[s][r] = fmaf(wv, fmaxf(acc[c][s][r] + ub, 0.f), zacc[s][r]);
        }
    }
    // the eight lanes of a half that share ab = lane & 3 hold the partial sums of one output pixel
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = zacc[s][r];
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64);
            v += __shfl_xor(v, 16, 64);
            if ((lane & 28) == 0) zs[wave][s * 32 + crow(r, half)][lane & 3] = v;
        }
    __syncthreads();
    float loss = 0.f;
    if (live) {
        float s = ((zs[0][opx][oab] + zs[1][opx][oab]) + zs[2][opx][oab]) + zs[3][opx][oab];
        if (bias) s += bias[lb];
        if (z) z[o] = s;
        if (target) {
            const float t = target[o];
            loss = bce_with_logits(s, t);
            if (g0) g0[o] = (sigmoidf(s) - t) * inv;
        }
    }
    if (row_loss) store_tile_loss<4>(loss, wl, row_loss + (int64_t)n * gridDim.x + blockIdx.x);
}

// g[n, :] * u of one RoI as sg[p][ab], zeros from pixel hw to pixel `fill`; u = up * inv_div
__device__ __forceinline__ void stage_g(const float* __restrict__ g, const float* __restrict__ up, const float* __restrict__ inv_div,
                                        int n, int w, int hw, int fill, float* sg) {
    const float u = upstream_scale(up, inv_div);
    for (int i = threadIdx.x; i < fill * 4; i += 256) {
        const int p = i >> 2;
        sg[i] = p < hw ? g[(int64_t)n * 4 * hw + out_pixel(p, i & 3, w)] * u : 0.f;
    }
}

// The backward's recomputation: block (column group, n) walks the pixel tiles of RoI n.  signs [n][ceil(hw / 32)][4 Co]: bit q
// of word (n, t, j) is pre[n, 32 t + q, j] > 0.  rows [n][co + 1] (nullable): sum_P g y per co, then sum_P g.
template <typename T>
__global__ void __launch_bounds__(256, 2) mask_tail_rows_kernel(const T* __restrict__ f, const float* __restrict__ upw,
                                                             const float* __restrict__ upb, const float* __restrict__ g,
                                                             const float* __restrict__ up, const float* __restrict__ inv_div,
                                                             const int64_t* __restrict__ labels, int C, int ci, int co, int w,
                                                             int hw, int valid_first, unsigned int* __restrict__ signs,
                                                             float* __restrict__ rows) {
    __shared__ float sA[kSlab * 64];
    __shared__ float sg[kMaxInHW * 4];
    __shared__ int slot[5];
    const int n = valid_first ? valid_first_roi(labels, gridDim.y, C, blockIdx.y, slot) : blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int64_t lb = labels[n];
    if (lb < 0 || lb >= C) return;                       // g counts as zero there: neither the bits nor the row are read
    const int ld = 4 * co, nsub32 = (hw + 31) / 32;
    const int j = blockIdx.x * 2 * kCols + wave * 32 + (lane & 31), ab = j & 3;
    const int ncl = blockIdx.x * 2 * kCols + kCols < ld ? 2 : 1;
    float ub[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int cidx = (j + c * kCols) >> 2;
        ub[c] = (cidx < co && upb) ? upb[cidx] : 0.f;
    }
    const T* fn = f + (int64_t)n * ci * hw;
    stage_g(g, up, inv_div, n, w, hw, hw, sg);           // (tail_gemm's first barrier publishes it)
    float stg[kSlab / 4];
    load_slab<T>(fn, ci, hw, 0, 0, stg);
    float rowacc[2] = {0.f, 0.f};
    for (int p0 = 0; p0 < hw; p0 += kPix) {
        const int nsub = min(2, (hw - p0 + 31) / 32);
        f32x16 acc[2][2];
        tail_gemm<T>(fn, upw, ci, ld, hw, p0, p0 + kPix, nsub, j, ncl, sA, stg, acc);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (s >= nsub || c >= ncl) continue;     // wave-uniform
                const int jc = j + c * kCols;
                unsigned int bits = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = crow(r, half), p = p0 + s * 32 + row;
                    const float pre = acc[c][s][r] + ub[c];
                    bits |= (pre > 0.f ? 1u : 0u) << row;
                    if (p < hw) rowacc[c] = fmaf(sg[p * 4 + ab], fmaxf(pre, 0.f), rowacc[c]);
                }
                bits |= __shfl_xor(bits, 32, 64);
                if (lane < 32 && jc < ld) signs[((int64_t)n * nsub32 + (p0 >> 5) + s) * ld + jc] = bits;
            }
    }
    if (!rows) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float v = rowacc[c];
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 32, 64);
        const int cidx = (j + c * kCols) >> 2;
        if ((lane & 35) == 0 && cidx < co) rows[(int64_t)n * (co + 1) + cidx] = v;
    }
    if (blockIdx.x == 0 && wave == 0) {
        float gs = 0.f;
        for (int i = lane; i < hw * 4; i += 64) gs += sg[i];
        gs = wave_sum(gs);
        if (lane == 0) rows[(int64_t)n * (co + 1) + co] = gs;
    }
}

// df[n, ci, p] = sum_j B[ci, j] dpre[n, p, j], dpre = g[n, P] weight[l, co] [pre > 0].  Block (64 pixels, n); a wave takes 32 ci
// at a time.  The sum over j runs in the order that lets a lane read four consecutive B values at once: lane half hf covers
// co = 2 t + hf in step t, one MFMA per ab.
template <typename T>
__global__ void __launch_bounds__(256) mask_tail_df_kernel(const float* __restrict__ g, const float* __restrict__ up,
                                                           const float* __restrict__ inv_div, const float* __restrict__ upw,
                                                           const float* __restrict__ weight, int64_t ld_w,
                                                           const int64_t* __restrict__ labels,
                                                           const unsigned int* __restrict__ signs, int C, int ci, int co, int w,
                                                           int hw, int valid_first, T* __restrict__ df) {
    __shared__ __attribute__((aligned(16))) unsigned int sbits[2][4 * kMaxC];
    __shared__ float sw[kMaxC];
    __shared__ int slot[5];
    const int n = valid_first ? valid_first_roi(labels, gridDim.y, C, blockIdx.y, slot) : blockIdx.y;
    const int p0 = blockIdx.x * kPix, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int li = lane & 31;
    const int64_t lb = labels[n];
    const int ld = 4 * co, nsub32 = (hw + 31) / 32, nsub = min(2, (hw - p0 + 31) / 32);
    T* dfn = df + (int64_t)n * ci * hw;
    if (lb < 0 || lb >= C) {                             // block-uniform: a zero slice
        const int px = tid & 63;
        if (p0 + px < hw)
            for (int c = tid >> 6; c < ci; c += 4) VT<T>::store1(dfn + (int64_t)c * hw + p0 + px, 0.f);
        return;
    }
    for (int c = tid; c < kMaxC; c += 256) sw[c] = c < co ? weight[lb * ld_w + c] : 0.f;
    const int fill = min(ld + 4, 4 * kMaxC);
    for (int s = 0; s < 2; ++s)
        for (int j = tid; j < fill; j += 256)
            sbits[s][j] = (s < nsub && j < ld) ? signs[((int64_t)n * nsub32 + (p0 >> 5) + s) * ld + j] : 0u;
    const float u = upstream_scale(up, inv_div);
    float g4[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) {
            const int p = p0 + s * 32 + li;
            g4[s][ab] = p < hw ? g[(int64_t)n * 4 * hw + out_pixel(p, ab, w)] * u : 0.f;
        }
    __syncthreads();
    const int steps = (co + 1) / 2;
    for (int cc = wave; cc * 32 < ci; cc += 4) {
        const int cidx = cc * 32 + li;
        const float* arow = upw + (int64_t)cidx * ld;
        f32x16 acc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
        for (int t = 0; t < steps; ++t) {
            const int c2 = 2 * t + half;
            f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
            if (cidx < ci && c2 < co) a4 = *reinterpret_cast<const f32x4*>(arow + 4 * c2);
            const float wv = sw[min(c2, kMaxC - 1)];
            const u32x4 b0 = *reinterpret_cast<const u32x4*>(&sbits[0][4 * min(c2, kMaxC - 1)]);
            const u32x4 b1 = *reinterpret_cast<const u32x4*>(&sbits[1][4 * min(c2, kMaxC - 1)]);
#pragma unroll
            for (int ab = 0; ab < 4; ++ab) {
                const float v0 = ((b0[ab] >> li) & 1u) ? g4[0][ab] * wv : 0.f;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[ab], v0, acc[0], 0, 0, 0);
                if (nsub > 1) {
                    const float v1 = ((b1[ab] >> li) & 1u) ? g4[1][ab] * wv : 0.f;
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[ab], v1, acc[1], 0, 0, 0);
                }
            }
        }
        for (int s = 0; s < nsub; ++s) {
            const int p = p0 + s * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = cc * 32 + crow(r, half);
                if (c < ci && p < hw) VT<T>::store1(dfn + (int64_t)c * hw + p, s ? acc[1][r] : acc[0][r]);
            }
        }
    }
}

// dup_weight partials: block (64 ci, 128 columns, RoI range) sums f^T dpre over the pixels of its RoIs in ascending order.
// partial [splits][ci][4 co], then colsum [splits][4 co]: the column sums of dpre, from which dup_bias follows.
template <typename T>
__global__ void __launch_bounds__(256) mask_tail_dup_kernel(const T* __restrict__ f, const float* __restrict__ g,
                                                            const float* __restrict__ up, const float* __restrict__ inv_div,
                                                            const float* __restrict__ weight, int64_t ld_w,
                                                            const int64_t* __restrict__ labels,
                                                            const unsigned int* __restrict__ signs, int N, int C, int ci, int co,
                                                            int w, int hw, int per, float* __restrict__ partial,
                                                            float* __restrict__ colsum) {
    __shared__ float sA[64 * 65];
    __shared__ float sg[kMaxInHW * 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, li = lane & 31;
    const int ci0 = blockIdx.x * 64, sp = blockIdx.z, ld = 4 * co, nsub32 = (hw + 31) / 32;
    const int j = blockIdx.y * kCols + wave * 32 + li, cidx = j >> 2, ab = j & 3;
    const bool jok = j < ld;
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
    float cs = 0.f;
    // (RoI, 64 pixels) rounds; the slab of f of the next round is asked for before this round's MFMAs and waits in registers
    const int n0 = sp * per, nslab = (hw + 63) / 64, total = (min(N, n0 + per) - n0) * nslab;
    const int spx = tid & 63, sc0 = tid >> 6;
    float stg[16];
    auto load = [&](int it) {
        const int n = n0 + it / nslab, q0 = (it % nslab) * 64;
        const T* fn = f + ((int64_t)n * ci + ci0) * hw + q0 + spx;
        const int64_t lb = labels[n];
        const bool pok = q0 + spx < hw && lb >= 0 && lb < C;     // f of an RoI outside is not read: its round is skipped below
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int c = rr * 4 + sc0;
            stg[rr] = (pok && ci0 + c < ci) ? VT<T>::load1(fn + (int64_t)c * hw) : 0.f;
        }
    };
    if (total > 0) load(0);
    for (int it = 0; it < total; ++it) {
        const int n = n0 + it / nslab, q0 = (it % nslab) * 64;
        const int64_t lb = labels[n];
        const bool valid = lb >= 0 && lb < C;            // block-uniform; an RoI outside contributes nothing
        __syncthreads();                                 // the previous round's reads of sA (and sg) are done
        if (q0 == 0 && valid) stage_g(g, up, inv_div, n, w, hw, nsub32 * 32, sg);
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) sA[(rr * 4 + sc0) * 65 + spx] = stg[rr];
        __syncthreads();
        if (it + 1 < total) load(it + 1);
        if (!valid) continue;
        const float wv = jok ? weight[lb * ld_w + cidx] : 0.f;
        for (int st = 0; st < 2; ++st) {
            const int q = q0 + st * 32;
            if (q >= hw) break;
            const unsigned int word = jok ? signs[((int64_t)n * nsub32 + (q >> 5)) * ld + j] : 0u;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int kp = 2 * s + half;
                const float b = ((word >> kp) & 1u) ? sg[(q + kp) * 4 + ab] * wv : 0.f;
                cs += b;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[li * 65 + st * 32 + kp], b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[(32 + li) * 65 + st * 32 + kp], b, acc[1], 0, 0, 0);
            }
        }
    }
    if (jok) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = ci0 + s * 32 + crow(r, half);
                if (c < ci) partial[((int64_t)sp * ci + c) * ld + j] = acc[s][r];
            }
    }
    cs += __shfl_xor(cs, 32, 64);
    if (blockIdx.x == 0 && lane < 32 && jok) colsum[(int64_t)sp * ld + j] = cs;
}

// the partials in range order: thread i < ci * 4 co one element of dup_weight, the co threads behind them dup_bias
__global__ void __launch_bounds__(256) mask_tail_dup_sum_kernel(const float* __restrict__ partial, const float* __restrict__ colsum,
                                                                int splits, int ci, int co, float* __restrict__ dupw,
                                                                float* __restrict__ dupb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)ci * 4 * co;
    if (i < total) {
        if (!dupw) return;
        float a = 0.f;
        for (int s = 0; s < splits; ++s) a += partial[s * total + i];
        dupw[i] = a;
    } else if (i < total + co && dupb) {
        const int c = (int)(i - total);
        float a = 0.f;
        for (int s = 0; s < splits; ++s) {
            const float* p = colsum + (int64_t)s * 4 * co + 4 * c;
            a += (p[0] + p[1]) + (p[2] + p[3]);
        }
        dupb[c] = a;
    }
}

inline bool geometry_ok(int n, int c, int ci, int co, int h, int w) {
    return rois_ok(n, c) && dim_ok(ci, kMaxC) && dim_ok(co, kMaxC) && h >= 1 && w >= 1 && (int64_t)h * w <= kMaxInHW;
}

// The forward of both entries.  inv_div == nullptr: the divisor 4 n hw is fixed here, g0 is stored divided and the row partials
// go through rows_reduce_kernel; otherwise g0 is stored undivided and mask_predict_finish_kernel writes *loss and *inv_div.
// The entries with a device divisor are the ones that meet padded rows: they (inv_div != nullptr, here and in the rows and df
// launchers) put the valid RoIs first in the grid (valid_first_roi).
int tail_fwd(const void* f, int dtype, const float* up_weight, const float* up_bias, const float* weight, int64_t ld_w,
             const float* bias, const int64_t* labels, const float* target, int n, int c, int ci, int co, int h, int w, int valid_rows,
             float* z, float* g0, float* row_loss, float* loss, float* inv_div, int* status, void* stream) {
    hipStream_t st = as_stream(stream);
    const int hw = h * w, tiles = (hw + kPix - 1) / kPix;
    const dim3 grid(tiles, n);
    const double invd = 1.0 / ((double)n * 4.0 * (double)hw);
    const float inv = inv_div ? 1.0f : (float)invd;
    float* rows = target ? row_loss : nullptr;
    dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((mask_tail_fwd_kernel<T>), grid, dim3(256), 0, st, (const T*)f, up_weight, up_bias, weight, ld_w, bias,
                           labels, target, c, ci, co, w, hw, inv, inv_div ? 1 : 0, z, g0, rows, status);
    });
    IIF_LAUNCH_CHECK();
    if (!target) return IIF_OK;
    if (inv_div)
        hipLaunchKernelGGL(mask_predict_finish_kernel, dim3(1), dim3(256), 0, st, row_loss, n * tiles, labels, n, c, 4 * hw,
                           valid_rows ? 1 : 0, loss, inv_div);
    else
        hipLaunchKernelGGL(rows_reduce_kernel<double>, dim3(1), dim3(256), 0, st, row_loss, n * tiles, invd, loss);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int tail_bwd_rows(const void* f, int dtype, const float* up_weight, const float* up_bias, const float* g, const float* up,
                  const float* inv_div, const int64_t* labels, int n, int c, int ci, int co, int h, int w, unsigned int* signs,
                  float* rows, void* stream) {
    if (!geometry_ok(n, c, ci, co, h, w) || !dtype_ok(dtype)) return IIF_EINVAL;
    if (!f || !up_weight || !g || !labels || !signs) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((4 * co + 2 * kCols - 1) / (2 * kCols), n);
    dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((mask_tail_rows_kernel<T>), grid, dim3(256), 0, st, (const T*)f, up_weight, up_bias, g, up, inv_div, labels,
                           c, ci, co, w, h * w, inv_div ? 1 : 0, signs, rows);
    });
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int tail_bwd_input(const float* g, const float* up, const float* inv_div, const float* up_weight, const float* weight, int64_t ld_w,
                   const int64_t* labels, const unsigned int* signs, int n, int c, int ci, int co, int h, int w, void* df, int dtype,
                   void* stream) {
    if (!geometry_ok(n, c, ci, co, h, w) || ld_w < co || !dtype_ok(dtype)) return IIF_EINVAL;
    if (!g || !up_weight || !weight || !labels || !signs || !df) return IIF_EINVAL;
    if ((uintptr_t)up_weight % 16) return IIF_EUNSUPPORTED;          // rows of 4 co floats are read 16 bytes at a time
    if (n == 0) return IIF_OK;
    hipStream_t st = as_stream(stream);
    const int hw = h * w;
    const dim3 grid((hw + kPix - 1) / kPix, n);
    dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((mask_tail_df_kernel<T>), grid, dim3(256), 0, st, g, up, inv_div, up_weight, weight, ld_w, labels, signs, c,
                           ci, co, w, hw, inv_div ? 1 : 0, (T*)df);
    });
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int tail_splits(int n, int ci, int co) {
    if (n < 1 || ci < 1 || co < 1) return 0;
    const int tiles = ((ci + 63) / 64) * ((4 * co + kCols - 1) / kCols);
    int s = 512 / tiles;
    s = s < 1 ? 1 : (s > 16 ? 16 : s);
    s = s > n ? n : s;
    const int per = (n + s - 1) / s;
    return (n + per - 1) / per;
}

int tail_bwd_params(const void* f, int dtype, const float* g, const float* up, const float* inv_div, const float* weight, int64_t ld_w,
                    const int64_t* labels, const unsigned int* signs, int n, int c, int ci, int co, int h, int w, float* partial,
                    float* dup_weight, float* dup_bias, void* stream) {
    if (!geometry_ok(n, c, ci, co, h, w) || ld_w < co || !dtype_ok(dtype)) return IIF_EINVAL;
    if (!f || !g || !weight || !labels || !signs || !partial || (!dup_weight && !dup_bias)) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    hipStream_t st = as_stream(stream);
    const int splits = tail_splits(n, ci, co), per = (n + splits - 1) / splits;
    const dim3 grid((ci + 63) / 64, (4 * co + kCols - 1) / kCols, splits);
    float* colsum = partial + (int64_t)splits * ci * 4 * co;
    dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((mask_tail_dup_kernel<T>), grid, dim3(256), 0, st, (const T*)f, g, up, inv_div, weight, ld_w, labels, signs,
                           n, c, ci, co, w, h * w, per, partial, colsum);
    });
    IIF_LAUNCH_CHECK();
    const int64_t total = (int64_t)ci * 4 * co + co;
    hipLaunchKernelGGL(mask_tail_dup_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, partial, colsum, splits, ci,
                       co, dup_weight, dup_bias);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // namespace

extern "C" {

int iif_mask_tail_fwd(const void* f, int dtype, const float* up_weight, const float* up_bias, const float* weight, int64_t ld_w,
                      const float* bias, const int64_t* labels, const float* target, int n, int c, int ci, int co, int h, int w,
                      float* z, float* g0, float* row_loss, float* loss, int* status, void* stream) {
    if (!geometry_ok(n, c, ci, co, h, w) || ld_w < co || !dtype_ok(dtype)) return IIF_EINVAL;
    if (!f || !up_weight || !weight || !labels || !status || (!z && !target)) return IIF_EINVAL;
    if (target ? (!row_loss || !loss) : (g0 != nullptr)) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    return tail_fwd(f, dtype, up_weight, up_bias, weight, ld_w, bias, labels, target, n, c, ci, co, h, w, 0, z, g0, row_loss, loss,
                    nullptr, status, stream);
}

int iif_mask_tail_bwd_rows(const void* f, int dtype, const float* up_weight, const float* up_bias, const float* g, const float* up,
                           const int64_t* labels, int n, int c, int ci, int co, int h, int w, unsigned int* signs, float* rows,
                           void* stream) {
    return tail_bwd_rows(f, dtype, up_weight, up_bias, g, up, nullptr, labels, n, c, ci, co, h, w, signs, rows, stream);
}

int iif_mask_tail_bwd_input(const float* g, const float* up, const float* up_weight, const float* weight, int64_t ld_w,
                            const int64_t* labels, const unsigned int* signs, int n, int c, int ci, int co, int h, int w, void* df,
                            int dtype, void* stream) {
    return tail_bwd_input(g, up, nullptr, up_weight, weight, ld_w, labels, signs, n, c, ci, co, h, w, df, dtype, stream);
}

int iif_mask_tail_splits(int n, int ci, int co) { return tail_splits(n, ci, co); }

int iif_mask_tail_bwd_params(const void* f, int dtype, const float* g, const float* up, const float* weight, int64_t ld_w,
                             const int64_t* labels, const unsigned int* signs, int n, int c, int ci, int co, int h, int w,
                             float* partial, float* dup_weight, float* dup_bias, void* stream) {
    return tail_bwd_params(f, dtype, g, up, nullptr, weight, ld_w, labels, signs, n, c, ci, co, h, w, partial, dup_weight, dup_bias,
                           stream);
}

int iif_mask_tail_bwd_classes(const float* rows, const int64_t* labels, int n, int c, int co, float* dweight, float* dbias,
                              void* stream) {
    if (!rois_ok(n, c) || !dim_ok(co, kMaxC)) return IIF_EINVAL;
    if (!rows || !labels || (!dweight && !dbias)) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    hipLaunchKernelGGL(mask_predict_dw_classes_kernel, dim3(c), dim3(256), 0, as_stream(stream), rows, labels, n, co, dweight, dbias);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_mask_tail_loss_fwd(const void* f, int dtype, const float* up_weight, const float* up_bias, const float* weight, int64_t ld_w,
                           const float* bias, const int64_t* labels, const float* target, int n, int c, int ci, int co, int h, int w,
                           int valid_rows, float* g, float* row_loss, float* loss, float* inv_div, void* stream) {
    if (!geometry_ok(n, c, ci, co, h, w) || ld_w < co || !dtype_ok(dtype)) return IIF_EINVAL;
    if (!f || !up_weight || !weight || !labels || !target || !row_loss || !loss || !inv_div) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    return tail_fwd(f, dtype, up_weight, up_bias, weight, ld_w, bias, labels, target, n, c, ci, co, h, w, valid_rows, nullptr, g,
                    row_loss, loss, inv_div, nullptr, stream);
}

int iif_mask_tail_loss_bwd_rows(const void* f, int dtype, const float* up_weight, const float* up_bias, const float* g,
                                const float* up, const float* inv_div, const int64_t* labels, int n, int c, int ci, int co, int h,
                                int w, unsigned int* signs, float* rows, void* stream) {
    return tail_bwd_rows(f, dtype, up_weight, up_bias, g, up, inv_div, labels, n, c, ci, co, h, w, signs, rows, stream);
}

int iif_mask_tail_loss_bwd_input(const float* g, const float* up, const float* inv_div, const float* up_weight, const float* weight,
                                 int64_t ld_w, const int64_t* labels, const unsigned int* signs, int n, int c, int ci, int co, int h,
                                 int w, void* df, int dtype, void* stream) {
    return tail_bwd_input(g, up, inv_div, up_weight, weight, ld_w, labels, signs, n, c, ci, co, h, w, df, dtype, stream);
}

int iif_mask_tail_loss_bwd_params(const void* f, int dtype, const float* g, const float* up, const float* inv_div,
                                  const float* weight, int64_t ld_w, const int64_t* labels, const unsigned int* signs, int n, int c,
                                  int ci, int co, int h, int w, float* partial, float* dup_weight, float* dup_bias, void* stream) {
    return tail_bwd_params(f, dtype, g, up, inv_div, weight, ld_w, labels, signs, n, c, ci, co, h, w, partial, dup_weight, dup_bias,
                           stream);
}

}  // extern "C"
