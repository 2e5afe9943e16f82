// What the class-selected mask predictor kernels share: the plain 1x1 predictor (mask_predictor.hip), its NormedConv2d variant
// (normed_mask_predictor.hip) and the fused mask head tail (mask_tail.hip).  Each piece exists once, here:
//   host    the argument checks and the (dtype, vector width) dispatch of the C entries
//   loads   VTn<T, V> (vec16.h): V consecutive elements of a channel row as floats
//   forward the weight-row staging, the group fold, the BCE term, the sigmoid, the fold of a tile's loss into its row partial and
//           the finishing kernel of the forwards whose divisor is a device scalar (row partials -> loss, valid-row count, 1 / divisor)
//   dweight the per-RoI row kernel of the two 1x1 predictors, the ascending list of a class's RoIs and the ordered sum of the
//           listed rows, the plain per-class kernel (scratch [n][cin + 1] -> dweight [C][cin], dbias [C])
// Every sum here has ONE order, which the callers' outputs depend on to the bit.
#pragma once
#include "common.h"
#include "vec16.h"

namespace {

// The 1x1 predictors.  kTile, pixels per forward block: 64, 128 or 256.  Measured at N = 256, 28 x 28, Cin = 256
// (profiles/mask_predictor.txt): 44 / 39 / 42 us with x in the Infinity Cache, no difference (83 .. 86 us) behind a 1 GiB fill
constexpr int kTile = 128;
static_assert(kTile == 64 || kTile == 128 || kTile == 256, "whole waves of pixels, at most the block");
constexpr int kChunk = 16;         // channels per block of the dx and dweight passes
constexpr int kMaxHW = 4096, kMaxCin = 2048;
// The Python wrappers size the row-partial buffer of every forward for tiles of kMinTile pixels (_TILE in mmdet_mask_predictor.py):
// the smallest tile any forward kernel may use.  A kernel with a larger tile leaves the end of that buffer unused.
constexpr int kMinTile = 64;
static_assert(kTile >= kMinTile, "the wrappers allocate one row partial per kMinTile pixels");
constexpr int kPiece = 2048;       // RoIs per piece of a class's list

inline bool dtype_ok(int dtype) { return dtype == IIF_F32 || dtype == IIF_BF16; }
// the part of the geometry every entry of the family checks: blockIdx.y carries the RoI
inline bool rois_ok(int n, int c) { return n >= 0 && n <= 65535 && c >= 1; }
inline bool dim_ok(int64_t v, int64_t most) { return v >= 1 && v <= most; }
inline bool geometry_ok(int n, int c, int cin, int hw) { return rois_ok(n, c) && dim_ok(cin, kMaxCin) && dim_ok(hw, kMaxHW); }
// 4 elements per lane: every channel row starts on a 4-element boundary
inline bool wide_ok(const void* p, int dtype, int hw) {
    return hw % 4 == 0 && ((uintptr_t)p % (4 * (uintptr_t)(dtype == IIF_F32 ? 4 : 2))) == 0;
}

// launch(T(), Width<V>()) with the element type of `dtype` (checked by dtype_ok) and V = 4 where `wide`, else 1
template <int V> struct Width { static constexpr int value = V; };
template <typename F> inline void dispatch_dtype(int dtype, F launch) {
    if (dtype == IIF_F32) launch(float()); else launch((unsigned short)0);
}
template <typename F> inline void dispatch_row(int dtype, bool wide, F launch) {
    dispatch_dtype(dtype, [&](auto t) { if (wide) launch(t, Width<4>()); else launch(t, Width<1>()); });
}

// Sum over the 256 threads of a block in a fixed order (butterfly inside a wave, the four waves in index order); every thread
// gets the sum.  red: 4 floats of LDS that nothing else uses until the next barrier after the call.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// |row|^2 of cin floats: thread t adds the squares of elements t, t + 256, ..., then block_sum.  The normed forward, dx pass and
// per-class pass all use this one order, so they agree on rho to the bit.
__device__ __forceinline__ float block_sumsq(const float* row, int cin, float* red) {
    float s = 0.f;
    for (int c = threadIdx.x; c < cin; c += 256) { const float w = row[c]; s = fmaf(w, w, s); }
    return block_sum(s, red);
}

// The selected weight row into LDS for the forward's channel loop; ends with the barrier that publishes it.
__device__ __forceinline__ void stage_weight_row(const float* __restrict__ wrow, int cin, float* sw) {
    for (int c = threadIdx.x; c < cin; c += 256) sw[c] = wrow[c];
    __syncthreads();
}
// The channel groups' partial sums of tile pixel p, added in group order.
template <int G> __device__ __forceinline__ float fold_groups(const float (&part)[G][kTile], int p) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) s += part[g][p];
    return s;
}
// binary_cross_entropy_with_logits of one logit, and the sigmoid its gradient (sigmoid(s) - t) needs
__device__ __forceinline__ float bce_with_logits(float s, float t) { return fmaxf(s, 0.f) - s * t + log1pf(expf(-fabsf(s))); }
__device__ __forceinline__ float sigmoidf(float s) { return 1.0f / (1.0f + expf(-s)); }
// A tile's loss terms, one per thread of the first kWaves waves of the block, into *out: butterfly inside a wave, the waves in
// index order through wl (kWaves floats of LDS).
template <int kWaves> __device__ __forceinline__ void store_tile_loss(float loss, float* wl, float* out) {
    const int tid = threadIdx.x;
    if (tid < kWaves * 64) {
        loss = wave_sum(loss);
        if ((tid & 63) == 0) wl[tid >> 6] = loss;
    }
    if (kWaves > 1) __syncthreads();
    if (tid == 0) {
        float tot = 0.f;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) tot += wl[i];
        *out = tot;
    }
}

// One block: the row partials summed in double in a fixed order, the divisor - n hw, or with valid_rows max(1, #{labels in
// [0, C)}) hw counted here - *loss = sum / divisor and *inv_div = 1 / divisor, the device scalar every backward pass multiplies in.
// hw: the pixels the loss averages over per RoI (the tail: 4 h w).
__global__ void __launch_bounds__(256) mask_predict_finish_kernel(const float* __restrict__ rows, int nrows,
                                                                  const int64_t* __restrict__ labels, int n, int C, int hw,
                                                                  int valid_rows, float* __restrict__ loss,
                                                                  float* __restrict__ inv_div) {
    __shared__ double sh[256];
    __shared__ int cnt[256];
    double acc = 0;
    int k = 0;
    for (int i = threadIdx.x; i < nrows; i += 256) acc += (double)rows[i];
    if (valid_rows)
        for (int i = threadIdx.x; i < n; i += 256) k += (labels[i] >= 0 && labels[i] < C) ? 1 : 0;
    sh[threadIdx.x] = acc;
    cnt[threadIdx.x] = k;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh[threadIdx.x] += sh[threadIdx.x + o];
            cnt[threadIdx.x] += cnt[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double rois = valid_rows ? (double)max(1, cnt[0]) : (double)n;
        const double inv = 1.0 / (rois * (double)hw);
        *loss = (float)(sh[0] * inv);
        *inv_div = (float)inv;
    }
}

// u = up * inv_div, the factor every backward kernel of the family applies to the stored gradient: two device scalars, either
// may be absent (an absent one multiplies by 1.0f, which changes no bit).
__device__ __forceinline__ float upstream_scale(const float* __restrict__ up, const float* __restrict__ inv_div) {
    return (up ? *up : 1.0f) * (inv_div ? *inv_div : 1.0f);
}

// The RoI that block y of a (., n) grid works on when the RoIs with a label in [0, C) go first: the y-th of them in ascending
// index or, for y >= K (their number), the RoI of rank n - 1 - y among the others - one pass, K is never needed.  What is computed
// for a RoI does not depend on the block that computes it, so no result changes; but the blocks with work are then the first in
// dispatch order and spread over the CUs as they do on compacted rows, where otherwise a CU may draw several of them and the
// grid waits for it (profiles/mask_valid_rows.txt).  The labels pass 256 at a time, a ballot and a prefix count rank each one,
// as in class_roi_list; exactly one RoI matches.  All 256 threads call it; slot: 5 ints of LDS of its own.
__device__ __forceinline__ int valid_first_roi(const int64_t* __restrict__ labels, int n, int C, int y, int* slot) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int before = 0;                                      // valid labels of the earlier rounds (block-uniform)
    if (tid == 0) slot[4] = -1;                          // (ordered before the matching thread's write by the round's barriers)
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool in = i < n;
        const int64_t lb = in ? labels[i] : -1;
        const bool hit = in && lb >= 0 && lb < C;
        const unsigned long long b = __ballot(hit);
        __syncthreads();
        if (lane == 0) slot[wv] = __popcll(b);
        __syncthreads();
        int rank = before;                               // valid labels before i
        for (int w = 0; w < wv; ++w) rank += slot[w];
        rank += __popcll(b & ((1ull << lane) - 1ull));
        if (in && (hit ? rank == y : i - rank == n - 1 - y)) slot[4] = i;
        before += slot[0] + slot[1] + slot[2] + slot[3];
    }
    __syncthreads();
    return slot[4];
}

// Rows of the weight gradient of the 1x1 predictors: block (chunk, n) stages u g of its RoI once - kNormed: u g A - with
// u = up * inv_div; 16 lanes per channel sum it against x over the contiguous pixels, a 16-lane butterfly folds them.
// scratch[n, c] for c < cin; scratch[n, cin] = u sum_p g (without A: kNormed keeps that copy in a second LDS array), the bias
// gradient's row.  ca is read by kNormed only.  valid_first: block y takes valid_first_roi(y) instead of RoI y.
template <typename T, int V, bool kNormed>
__global__ void __launch_bounds__(256) mask_predict_dw_rows_kernel(const T* __restrict__ x, const float* __restrict__ g,
                                                                   const float* __restrict__ ca, const float* __restrict__ up,
                                                                   const float* __restrict__ inv_div,
                                                                   const int64_t* __restrict__ labels, int C, int cin, int hw,
                                                                   int valid_first, float* __restrict__ scratch) {
    __shared__ __attribute__((aligned(16))) float sg[kMaxHW];
    __shared__ int slot[5];
    float* s0 = sg;                                      // what the bias column sums
    if constexpr (kNormed) {
        __shared__ float unscaled[kMaxHW];
        s0 = unscaled;
    }
    const int n = valid_first ? valid_first_roi(labels, gridDim.y, C, blockIdx.y, slot) : blockIdx.y;
    const int c0 = blockIdx.x * kChunk, tid = threadIdx.x;
    const int64_t lb = labels[n];
    if (lb < 0 || lb >= C) return;                       // no class reads this RoI's row
    const float u = upstream_scale(up, inv_div);
    for (int p = tid; p < hw; p += 256) {
        const int64_t o = (int64_t)n * hw + p;
        const float gu = g[o] * u;
        if constexpr (kNormed) {
            sg[p] = gu * ca[o];
            if (blockIdx.x == 0) s0[p] = gu;
        } else {
            sg[p] = gu;
        }
    }
    __syncthreads();
    const int c = c0 + (tid >> 4), l16 = tid & 15;
    const int per = hw / V;
    float acc = 0.f, gs = 0.f;
    if (c < cin) {
        const T* xp = x + ((int64_t)n * cin + c) * hw;
#pragma unroll 4
        for (int i = l16; i < per; i += 16) {
            float v[V];
            VTn<T, V>::load(xp + i * V, v);
#pragma unroll
            for (int j = 0; j < V; ++j) acc = fmaf(sg[i * V + j], v[j], acc);
        }
    }
    if (blockIdx.x == 0)                                 // (block-uniform)
        for (int i = l16; i < hw; i += 16) gs += s0[i];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        gs += __shfl_xor(gs, o, 64);
    }
    float* row = scratch + (int64_t)n * (cin + 1);
    if (l16 == 0 && c < cin) row[c] = acc;
    if (blockIdx.x == 0 && tid == 0) row[cin] = gs;
}

// The ascending list of the RoIs n0 .. n0 + m - 1 (m <= kPiece) whose label is k, by all 256 threads of the block: the labels
// pass 256 at a time, a ballot and a prefix count place every hit (no sort).  list: kPiece ints of LDS, wcnt: 4; returns the
// block-uniform length.  Two barriers per round: the first lets the previous round's reads of wcnt - and, in the first round,
// the caller's reads of the previous piece's list - finish before either is written again; the closing barrier publishes the list.
__device__ __forceinline__ int class_roi_list(const int64_t* __restrict__ labels, int n0, int m, int k, int* list, int* wcnt) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int cnt = 0;                                         // block-uniform
    for (int i0 = 0; i0 < m; i0 += 256) {
        const int i = i0 + tid;
        const bool hit = i < m && labels[n0 + i] == k;
        const unsigned long long b = __ballot(hit);
        __syncthreads();
        if (lane == 0) wcnt[wv] = __popcll(b);
        __syncthreads();
        int off = cnt;
        for (int w = 0; w < wv; ++w) off += wcnt[w];
        if (hit) list[off + __popcll(b & ((1ull << lane) - 1ull))] = n0 + i;
        cnt += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
    __syncthreads();
    return cnt;
}
// acc + the elements sc[list[j] * ld], j = 0 .. cnt - 1, added in list order, eight loads in flight
__device__ __forceinline__ float add_listed_rows(const float* __restrict__ sc, int ld, const int* list, int cnt, float acc) {
    int j = 0;
    for (; j + 8 <= cnt; j += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = sc[(int64_t)list[j + u] * ld];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; j < cnt; ++j) acc += sc[(int64_t)list[j] * ld];
    return acc;
}

// One block per class: every thread adds the scratch rows of the class's RoIs for its column, in ascending RoI index; columns
// outside pieces, so a round of 256 columns rebuilds the lists.  Writes every row of dweight and every element of dbias.
__global__ void __launch_bounds__(256) mask_predict_dw_classes_kernel(const float* __restrict__ scratch,
                                                                      const int64_t* __restrict__ labels, int n, int cin,
                                                                      float* __restrict__ dweight, float* __restrict__ dbias) {
    __shared__ int list[kPiece];
    __shared__ int wcnt[4];
    const int k = blockIdx.x, ld = cin + 1;
    for (int col0 = 0; col0 < ld; col0 += 256) {
        const int col = col0 + threadIdx.x;
        float acc = 0.f;
        for (int n0 = 0; n0 < n; n0 += kPiece) {
            const int cnt = class_roi_list(labels, n0, min(kPiece, n - n0), k, list, wcnt);
            if (col < ld) acc = add_listed_rows(scratch + col, ld, list, cnt, acc);
        }
        if (col < cin) { if (dweight) dweight[(int64_t)k * cin + col] = acc; }
        else if (col == cin) { if (dbias) dbias[k] = acc; }
    }
}

}  // namespace
