// The class-selected mask predictor of the Mask R-CNN head, gfx950: conv_logits evaluated at each RoI's label only.
//
// Reference: FCNMaskHead.forward ends with mask_pred = conv_logits(x), a 1x1 convolution to num_classes channels
// (fcn_mask_head.py:127-136); mask_cross_entropy keeps pred[inds, label] (cross_entropy_loss.py:158-162) and get_seg_masks
// mask_pred[range(N), labels] (fcn_mask_head.py:289-290): one channel per RoI.  The gradient of every other channel is exactly
// zero, so the [N, C, H, W] logits (966 MB at the LVIS training shape) are never formed:
//   forward   z[n, p] = bias[l] + sum_c weight[l, c] x[n, c, p],  l = labels[n]; with targets the BCE rows, the mean and the
//             compact gradient g0 = (sigmoid(z) - t) / (N HW) as [N, HW]
//   dx        g[n, p] weight[l, c], every element written once
//   dweight   per-RoI rows sum_p g[n, p] x[n, c, p] (+ sum_p g[n, p]) into a scratch [N, Cin + 1], then one block per class adds
//             the rows of its RoIs in ascending RoI index and writes EVERY row of dweight / dbias (zeros where no RoI has it)
// All three stream x or dx once (bandwidth-bound, no matrix pipe), accumulate in fp32 in a fixed order and use no float atomics:
// bit-identical from call to call.  The iif_mask_predict_loss_* entries leave the divisor to the device: the forward stores
// g = sigmoid(z) - t undivided, mask_predict_finish_kernel counts the valid rows and writes *inv_div, and the backward kernels
// multiply by u = up * inv_div.  x and dx are NCHW-contiguous; a channel row is loaded 4 elements per lane where HW is a
// multiple of 4 and the base is aligned to 4 elements, one element per lane otherwise (HW = 63: rows 252 bytes apart).
#include "common.h"
#include "loss_reduce.h"
#include "mask_predict_core.h"

namespace {

// Forward: block (tile, n) owns kTile pixels of RoI n.  Lanes 0 .. 64 / V - 1 of a channel group cover the tile V pixels each,
// the 256 V / kTile groups of the block take the channels g, g + 256 V / kTile, ...; the groups' partial sums are folded through LDS in group order
// before the bias and the BCE, which need the complete channel sum.  row_loss holds one partial per block.  inv: the factor
// stored into g0, 1 / (n hw) or 1.0f where the divisor is a device scalar.  status: nullable.  valid_first (here and in the dx
// kernel): block y takes valid_first_roi(y) instead of RoI y.
template <typename T, int V>
__global__ void __launch_bounds__(256) mask_predict_fwd_kernel(const T* __restrict__ x, const float* __restrict__ weight, int64_t ld_w,
                                                               const float* __restrict__ bias, const int64_t* __restrict__ labels,
                                                               const float* __restrict__ target, int C, int cin, int hw, float inv,
                                                               int valid_first, float* __restrict__ z, float* __restrict__ g0,
                                                               float* __restrict__ row_loss, int* status) {
    constexpr int LPG = kTile / V, G = 256 / LPG;        // lanes per channel group, channel groups
    __shared__ float sw[kMaxCin];
    __shared__ float part[G][kTile];
    __shared__ float wl[kTile / 64];
    __shared__ int slot[5];
    const int n = valid_first ? valid_first_roi(labels, gridDim.y, C, blockIdx.y, slot) : blockIdx.y;
    const int p0 = blockIdx.x * kTile, tid = threadIdx.x;
    const int64_t lb = labels[n];
    if (lb < 0 || lb >= C) {                             // block-uniform
        if (tid == 0) {
            if (status) atomicOr(status, 1);
            if (row_loss) row_loss[(int64_t)n * gridDim.x + blockIdx.x] = 0.f;
        }
        if (tid < kTile && p0 + tid < hw) {
            if (z) z[(int64_t)n * hw + p0 + tid] = 0.f;
            if (g0) g0[(int64_t)n * hw + p0 + tid] = 0.f;
        }
        return;
    }
    stage_weight_row(weight + lb * ld_w, cin, sw);
    const int grp = tid / LPG, pl = (tid % LPG) * V;     // pixel offset of this lane inside the tile
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    if (p0 + pl < hw) {                                  // (V == 4: hw is a multiple of 4, a vector is inside or outside as a whole)
        const T* xp = x + (int64_t)n * cin * hw + p0 + pl;
#pragma unroll 8
        for (int c = grp; c < cin; c += G) {
            float v[V];
            VTn<T, V>::load(xp + (int64_t)c * hw, v);
            const float wc = sw[c];
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = fmaf(wc, v[j], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) part[grp][pl + j] = acc[j];
    __syncthreads();
    float loss = 0.f;
    if (tid < kTile && p0 + tid < hw) {
        float s = fold_groups(part, tid);
        if (bias) s += bias[lb];
        const int64_t o = (int64_t)n * hw + p0 + tid;
        if (z) z[o] = s;
        if (target) {
            const float t = target[o];
            loss = bce_with_logits(s, t);
            if (g0) g0[o] = (sigmoidf(s) - t) * inv;
        }
    }
    if (row_loss) store_tile_loss<kTile / 64>(loss, wl, row_loss + (int64_t)n * gridDim.x + blockIdx.x);
}

// dx = g * u * weight[l, :], u = up * inv_div: block (chunk, n) writes the contiguous kChunk * hw elements of channels
// [c0, c0 + kChunk) of RoI n.
template <typename T, int V>
__global__ void __launch_bounds__(256) mask_predict_dx_kernel(const float* __restrict__ g, const float* __restrict__ up,
                                                              const float* __restrict__ inv_div,
                                                              const float* __restrict__ weight, int64_t ld_w,
                                                              const int64_t* __restrict__ labels, int C, int cin, int hw,
                                                              int valid_first, T* __restrict__ dx) {
    __shared__ __attribute__((aligned(16))) float sg[kMaxHW];
    __shared__ float sw[kChunk];
    __shared__ int slot[5];
    const int n = valid_first ? valid_first_roi(labels, gridDim.y, C, blockIdx.y, slot) : blockIdx.y;
    const int c0 = blockIdx.x * kChunk, tid = threadIdx.x;
    const int nc = min(kChunk, cin - c0);
    const int64_t lb = labels[n];
    const bool ok = lb >= 0 && lb < C;
    const float u = upstream_scale(up, inv_div);
    for (int p = tid; p < hw; p += 256) sg[p] = ok ? g[(int64_t)n * hw + p] * u : 0.f;
    if (tid < kChunk) sw[tid] = (ok && tid < nc) ? weight[lb * ld_w + c0 + tid] : 0.f;
    __syncthreads();
    T* out = dx + ((int64_t)n * cin + c0) * hw;
    const int per = hw / V, total = nc * per;
    for (int i = tid; i < total; i += 256) {
        const int c = i / per, p = (i - c * per) * V;
        const float wc = sw[c];
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = sg[p + j] * wc;
        VTn<T, V>::store(out + (int64_t)i * V, v);
    }
}

// dweight / dbias: mask_predict_dw_rows_kernel<T, V, false> and mask_predict_dw_classes_kernel of mask_predict_core.h.

// The forward of both entries.  inv_div == nullptr: the divisor n hw is fixed here, g0 is stored divided and the row partials
// go through rows_reduce_kernel; otherwise g0 is stored undivided and mask_predict_finish_kernel writes *loss and *inv_div.
// The entries with a device divisor are the ones that meet padded rows: they (inv_div != nullptr, here and in the two backward
// launchers) put the valid RoIs first in the grid.
int predict_fwd(const void* x, int dtype, const float* weight, int64_t ld_w, const float* bias, const int64_t* labels,
                const float* target, int n, int c, int cin, int hw, int valid_rows, float* z, float* g0, float* row_loss, float* loss,
                float* inv_div, int* status, void* stream) {
    hipStream_t st = as_stream(stream);
    const int tiles = (hw + kTile - 1) / kTile;
    const dim3 grid(tiles, n);
    const double invd = 1.0 / ((double)n * (double)hw);
    const float inv = inv_div ? 1.0f : (float)invd;
    float* rows = target ? row_loss : nullptr;
    dispatch_row(dtype, wide_ok(x, dtype, hw), [&](auto t, auto v) {
        using T = decltype(t);
        hipLaunchKernelGGL((mask_predict_fwd_kernel<T, decltype(v)::value>), grid, dim3(256), 0, st, (const T*)x, weight, ld_w, bias,
                           labels, target, c, cin, hw, inv, inv_div ? 1 : 0, z, g0, rows, status);
    });
    IIF_LAUNCH_CHECK();
    if (!target) return IIF_OK;
    if (inv_div)
        hipLaunchKernelGGL(mask_predict_finish_kernel, dim3(1), dim3(256), 0, st, row_loss, n * tiles, labels, n, c, hw,
                           valid_rows ? 1 : 0, loss, inv_div);
    else
        hipLaunchKernelGGL(rows_reduce_kernel<double>, dim3(1), dim3(256), 0, st, row_loss, n * tiles, invd, loss);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int predict_bwd_input(const float* g, const float* up, const float* inv_div, const float* weight, int64_t ld_w, const int64_t* labels,
                      int n, int c, int cin, int hw, void* dx, int dtype, void* stream) {
    if (!geometry_ok(n, c, cin, hw) || ld_w < cin || !dtype_ok(dtype)) return IIF_EINVAL;
    if (!g || !weight || !labels || !dx) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((cin + kChunk - 1) / kChunk, n);
    dispatch_row(dtype, wide_ok(dx, dtype, hw), [&](auto t, auto v) {
        using T = decltype(t);
        hipLaunchKernelGGL((mask_predict_dx_kernel<T, decltype(v)::value>), grid, dim3(256), 0, st, g, up, inv_div, weight, ld_w,
                           labels, c, cin, hw, inv_div ? 1 : 0, (T*)dx);
    });
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int predict_bwd_weight(const void* x, int dtype, const float* g, const float* up, const float* inv_div, const int64_t* labels, int n,
                       int c, int cin, int hw, float* scratch, float* dweight, float* dbias, void* stream) {
    if (!geometry_ok(n, c, cin, hw) || !dtype_ok(dtype)) return IIF_EINVAL;
    if (!x || !g || !labels || !scratch || (!dweight && !dbias)) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((cin + kChunk - 1) / kChunk, n);
    dispatch_row(dtype, wide_ok(x, dtype, hw), [&](auto t, auto v) {
        using T = decltype(t);
        hipLaunchKernelGGL((mask_predict_dw_rows_kernel<T, decltype(v)::value, false>), grid, dim3(256), 0, st, (const T*)x, g,
                           (const float*)nullptr, up, inv_div, labels, c, cin, hw, inv_div ? 1 : 0, scratch);
    });
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(mask_predict_dw_classes_kernel, dim3(c), dim3(256), 0, st, scratch, labels, n, cin, dweight, dbias);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // namespace

extern "C" {

int iif_mask_predict_fwd(const void* x, int dtype, const float* weight, int64_t ld_w, const float* bias, const int64_t* labels,
                         const float* target, int n, int c, int cin, int hw, float* z, float* g0, float* row_loss, float* loss,
                         int* status, void* stream) {
    if (!geometry_ok(n, c, cin, hw) || ld_w < cin || !dtype_ok(dtype)) return IIF_EINVAL;
    if (!x || !weight || !labels || !status || (!z && !target)) return IIF_EINVAL;
    if (target ? (!row_loss || !loss) : (g0 != nullptr)) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    return predict_fwd(x, dtype, weight, ld_w, bias, labels, target, n, c, cin, hw, 0, z, g0, row_loss, loss, nullptr, status, stream);
}

int iif_mask_predict_bwd_input(const float* g, const float* up, const float* weight, int64_t ld_w, const int64_t* labels, int n,
                               int c, int cin, int hw, void* dx, int dtype, void* stream) {
    return predict_bwd_input(g, up, nullptr, weight, ld_w, labels, n, c, cin, hw, dx, dtype, stream);
}

int iif_mask_predict_bwd_weight(const void* x, int dtype, const float* g, const float* up, const int64_t* labels, int n, int c,
                                int cin, int hw, float* scratch, float* dweight, float* dbias, void* stream) {
    return predict_bwd_weight(x, dtype, g, up, nullptr, labels, n, c, cin, hw, scratch, dweight, dbias, stream);
}

int iif_mask_predict_loss_fwd(const void* x, int dtype, const float* weight, int64_t ld_w, const float* bias, const int64_t* labels,
                              const float* target, int n, int c, int cin, int hw, int valid_rows, float* g, float* row_loss,
                              float* loss, float* inv_div, void* stream) {
    if (!geometry_ok(n, c, cin, hw) || ld_w < cin || !dtype_ok(dtype)) return IIF_EINVAL;
    if (!x || !weight || !labels || !target || !row_loss || !loss || !inv_div) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    return predict_fwd(x, dtype, weight, ld_w, bias, labels, target, n, c, cin, hw, valid_rows, nullptr, g, row_loss, loss, inv_div,
                       nullptr, stream);
}

int iif_mask_predict_loss_bwd_input(const float* g, const float* up, const float* inv_div, const float* weight, int64_t ld_w,
                                    const int64_t* labels, int n, int c, int cin, int hw, void* dx, int dtype, void* stream) {
    return predict_bwd_input(g, up, inv_div, weight, ld_w, labels, n, c, cin, hw, dx, dtype, stream);
}

int iif_mask_predict_loss_bwd_weight(const void* x, int dtype, const float* g, const float* up, const float* inv_div,
                                     const int64_t* labels, int n, int c, int cin, int hw, float* scratch, float* dweight,
                                     float* dbias, void* stream) {
    return predict_bwd_weight(x, dtype, g, up, inv_div, labels, n, c, cin, hw, scratch, dweight, dbias, stream);
}

}  // extern "C"
