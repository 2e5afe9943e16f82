// The class-selected mask predictor of the cosine-norm heads, gfx950: NormedConv2d's conv_logits at each RoI's label only.
//
// Reference: predictor_cfg=dict(type='NormedConv2d', tempearture=20) puts normed_predictor.py:104-124 at the end of FCNMaskHead:
// the weight is normalised per output row, the input per pixel over its channels - neither depends on any OTHER class - and
// mask_cross_entropy / get_seg_masks keep one channel per RoI.  So, as in mask_predictor.hip, the gradient of every unselected
// class row is exactly zero and the [N, C, H, W] logits are never formed.  With l = labels[n], T = tempearture, q = power,
//   r = |x[n, :, p]|_2, rho = |w[l, :]|_2, s_x = T / (r^q + eps), s_w = 1 / (rho^q + eps), what = w[l] s_w, d = <what, x[n, :, p]>
//   forward   z[n, p] = s_x d + bias[l]; with targets the BCE rows, the loss, g = sigmoid(z) - t (UNSCALED: the divisor is a
//             device scalar, see mask_predict_finish_kernel) and the two coefficients A = s_x, B = d T q r^(q-2) / (r^q + eps)^2 (0 at r = 0)
//   dx        g (A what[c] - B x[n, c, p]): reads x once, writes dx once
//   dweight   per-RoI rows sum_p g A x (+ sum_p g) into a scratch [N, Cin + 1]; one block per class adds the rows of its RoIs in
//             ascending RoI index and applies the backward of the row normalisation; EVERY row of dweight / dbias is written
// Everything is fp32 in a fixed order without float atomics (the same bits from call to call), nothing of size [N, Cin, HW] is
// stored, nothing is read back.  power == 1 (every config) never calls powf.  x and dx are NCHW-contiguous, 4 elements per lane
// where HW is a multiple of 4 and the base is aligned, one otherwise.
#include "common.h"
#include "mask_predict_core.h"

namespace {

// v^q; power == 1 takes the path without powf
__device__ __forceinline__ float powq(float v, float q) { return q == 1.0f ? v : powf(v, q); }
// d q v^(q-2) / (v^q + eps)^2 for v > 0: the projection term of the normalisation's backward (d / v first: it is bounded)
__device__ __forceinline__ float back_coef(float d, float v, float q, float eps) {
    const float den = powq(v, q) + eps;
    return q == 1.0f ? (d / v) / (den * den) : d * q * powf(v, q - 2.0f) / (den * den);
}

// Forward: block (tile, n) owns kTile pixels of RoI n, as mask_predict_fwd_kernel; each channel group carries sum w x AND
// sum x^2 per pixel, both folded through LDS in group order.  The block computes rho of its own label row.
template <typename T, int V>
__global__ void __launch_bounds__(256) normed_predict_fwd_kernel(const T* __restrict__ x, const float* __restrict__ weight, int64_t ld_w,
                                                                 const float* __restrict__ bias, const int64_t* __restrict__ labels,
                                                                 const float* __restrict__ target, int C, int cin, int hw, float temp,
                                                                 float q, float eps, float* __restrict__ z, float* __restrict__ g,
                                                                 float* __restrict__ ca, float* __restrict__ cb,
                                                                 float* __restrict__ row_loss) {
    constexpr int LPG = kTile / V, G = 256 / LPG;        // lanes per channel group, channel groups
    __shared__ float sw[kMaxCin];
    __shared__ float part[2][G][kTile];
    __shared__ float red[4];
    __shared__ float wl[kTile / 64];
    const int n = blockIdx.y, p0 = blockIdx.x * kTile, tid = threadIdx.x;
    const int64_t lb = labels[n];
    if (lb < 0 || lb >= C) {                             // block-uniform; x of this RoI is not read
        if (tid == 0 && row_loss) row_loss[(int64_t)n * gridDim.x + blockIdx.x] = 0.f;
        if (tid < kTile && p0 + tid < hw) {
            const int64_t o = (int64_t)n * hw + p0 + tid;
            if (z) z[o] = 0.f;
            if (g) g[o] = 0.f;
            if (ca) ca[o] = 0.f;
            if (cb) cb[o] = 0.f;
        }
        return;
    }
    stage_weight_row(weight + lb * ld_w, cin, sw);
    const float rho = sqrtf(block_sumsq(sw, cin, red));
    const float s_w = 1.0f / (powq(rho, q) + eps);
    const int grp = tid / LPG, pl = (tid % LPG) * V;     // pixel offset of this lane inside the tile
    float acc[V], sq[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = sq[j] = 0.f;
    if (p0 + pl < hw) {                                  // (V == 4: hw is a multiple of 4, a vector is inside or outside as a whole)
        const T* xp = x + (int64_t)n * cin * hw + p0 + pl;
#pragma unroll 8
        for (int c = grp; c < cin; c += G) {
            float v[V];
            VTn<T, V>::load(xp + (int64_t)c * hw, v);
            const float wc = sw[c];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                acc[j] = fmaf(wc, v[j], acc[j]);
                sq[j] = fmaf(v[j], v[j], sq[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        part[0][grp][pl + j] = acc[j];
        part[1][grp][pl + j] = sq[j];
    }
    __syncthreads();
    float loss = 0.f;
    if (tid < kTile && p0 + tid < hw) {
        const float d = fold_groups(part[0], tid) * s_w;
        const float r = sqrtf(fold_groups(part[1], tid));
        const float s_x = temp / (powq(r, q) + eps);
        float s = s_x * d;
        if (bias) s += bias[lb];
        const int64_t o = (int64_t)n * hw + p0 + tid;
        if (z) z[o] = s;
        if (ca) ca[o] = s_x;
        if (cb) cb[o] = r > 0.f ? temp * back_coef(d, r, q, eps) : 0.f;
        if (target) {
            const float t = target[o];
            loss = bce_with_logits(s, t);
            if (g) g[o] = sigmoidf(s) - t;
        }
    }
    if (row_loss) store_tile_loss<kTile / 64>(loss, wl, row_loss + (int64_t)n * gridDim.x + blockIdx.x);
}

// The loss, the valid-row count and the divisor: mask_predict_finish_kernel of mask_predict_core.h.

// dx = u g (A what[c] - B x): block (chunk, n) reads and writes the contiguous kChunk * hw elements of channels
// [c0, c0 + kChunk) of RoI n; u = up * inv_div (device scalars, either may be absent).  A RoI with a label outside [0, C) gets
// zeros and its x is not read.
template <typename T, int V>
__global__ void __launch_bounds__(256) normed_predict_dx_kernel(const T* __restrict__ x, const float* __restrict__ g,
                                                                const float* __restrict__ ca, const float* __restrict__ cb,
                                                                const float* __restrict__ up, const float* __restrict__ inv_div,
                                                                const float* __restrict__ weight, int64_t ld_w,
                                                                const int64_t* __restrict__ labels, int C, int cin, int hw, float q,
                                                                float eps, T* __restrict__ dx) {
    __shared__ __attribute__((aligned(16))) float sa[kMaxHW];
    __shared__ __attribute__((aligned(16))) float sb[kMaxHW];
    __shared__ float swc[kChunk];
    __shared__ float red[4];
    const int n = blockIdx.y, c0 = blockIdx.x * kChunk, tid = threadIdx.x;
    const int nc = min(kChunk, cin - c0);
    const int64_t lb = labels[n];
    const bool ok = lb >= 0 && lb < C;                   // block-uniform
    T* out = dx + ((int64_t)n * cin + c0) * hw;
    const int per = hw / V, total = nc * per;
    if (!ok) {
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = 0.f;
        for (int i = tid; i < total; i += 256) VTn<T, V>::store(out + (int64_t)i * V, v);
        return;
    }
    const float u = upstream_scale(up, inv_div);
    for (int p = tid; p < hw; p += 256) {
        const int64_t o = (int64_t)n * hw + p;
        const float gu = g[o] * u;
        sa[p] = gu * ca[o];
        sb[p] = gu * cb[o];
    }
    const float* wrow = weight + lb * ld_w;
    const float rho = sqrtf(block_sumsq(wrow, cin, red));
    const float s_w = 1.0f / (powq(rho, q) + eps);
    if (tid < kChunk) swc[tid] = tid < nc ? wrow[c0 + tid] * s_w : 0.f;
    __syncthreads();
    const T* in = x + ((int64_t)n * cin + c0) * hw;
    for (int i = tid; i < total; i += 256) {
        const int c = i / per, p = (i - c * per) * V;
        const float wc = swc[c];
        float v[V];
        VTn<T, V>::load(in + (int64_t)i * V, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = fmaf(-sb[p + j], v[j], sa[p + j] * wc);
        VTn<T, V>::store(out + (int64_t)i * V, v);
    }
}

// The per-RoI rows of the weight gradient: mask_predict_dw_rows_kernel<T, V, true> of mask_predict_core.h.

// One block per class k: the ascending list of the class's RoIs (class_roi_list, 2048 labels at a time; pieces outside columns,
// so every list is built once), dwhat[k] = the sum of their scratch rows in list order (add_listed_rows), kept in LDS, then
//   dweight[k] = s_w dwhat - (<dwhat, w[k]> q rho^(q-2) / (rho^q + eps)^2) w[k]      (no second term where rho == 0)
// and dbias[k] = the sum of column cin.  A class no RoI has gets zeros without a look at its weights.
__global__ void __launch_bounds__(256) normed_predict_dw_classes_kernel(const float* __restrict__ scratch,
                                                                        const int64_t* __restrict__ labels,
                                                                        const float* __restrict__ weight, int64_t ld_w, int n,
                                                                        int cin, float q, float eps, float* __restrict__ dweight,
                                                                        float* __restrict__ dbias) {
    __shared__ int list[kPiece];
    __shared__ int wcnt[4];
    __shared__ float dwh[kMaxCin + 1];
    __shared__ float red[2][4];
    const int k = blockIdx.x, tid = threadIdx.x, ld = cin + 1;
    for (int col = tid; col < ld; col += 256) dwh[col] = 0.f;    // each thread owns its columns: no barrier needed for dwh
    int total = 0;                                       // block-uniform
    for (int n0 = 0; n0 < n; n0 += kPiece) {
        const int cnt = class_roi_list(labels, n0, min(kPiece, n - n0), k, list, wcnt);
        total += cnt;
        for (int col = tid; col < ld; col += 256) dwh[col] = add_listed_rows(scratch + col, ld, list, cnt, dwh[col]);
    }
    if (dbias && tid == (cin & 255)) dbias[k] = total ? dwh[cin] : 0.f;      // the owner of column cin
    if (!dweight) return;
    if (total == 0) {
        for (int col = tid; col < cin; col += 256) dweight[(int64_t)k * cin + col] = 0.f;
        return;
    }
    const float* wrow = weight + k * ld_w;
    const float rho = sqrtf(block_sumsq(wrow, cin, red[0]));
    float dot = 0.f;
    for (int col = tid; col < cin; col += 256) dot = fmaf(dwh[col], wrow[col], dot);
    dot = block_sum(dot, red[1]);
    const float s_w = 1.0f / (powq(rho, q) + eps);
    const float coef = rho > 0.f ? back_coef(dot, rho, q, eps) : 0.f;
    for (int col = tid; col < cin; col += 256) dweight[(int64_t)k * cin + col] = fmaf(-coef, wrow[col], s_w * dwh[col]);
}

}  // namespace

extern "C" {

int iif_normed_mask_predict_fwd(const void* x, int dtype, const float* weight, int64_t ld_w, const float* bias, const int64_t* labels,
                                const float* target, int n, int c, int cin, int hw, float temperature, float power, float eps,
                                int valid_rows, float* z, float* g, float* coef_a, float* coef_b, float* row_loss, float* loss,
                                float* inv_div, void* stream) {
    if (!geometry_ok(n, c, cin, hw) || ld_w < cin || !dtype_ok(dtype) || !(power > 0.f)) return IIF_EINVAL;
    if (!x || !weight || !labels || (!z && !target)) return IIF_EINVAL;
    if (target ? (!row_loss || !loss || !inv_div) : (g != nullptr)) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    hipStream_t st = as_stream(stream);
    const int tiles = (hw + kTile - 1) / kTile;
    const dim3 grid(tiles, n);
    float* rows = target ? row_loss : nullptr;
    dispatch_row(dtype, wide_ok(x, dtype, hw), [&](auto t, auto v) {
        using T = decltype(t);
        hipLaunchKernelGGL((normed_predict_fwd_kernel<T, decltype(v)::value>), grid, dim3(256), 0, st, (const T*)x, weight, ld_w, bias,
                           labels, target, c, cin, hw, temperature, power, eps, z, g, coef_a, coef_b, rows);
    });
    IIF_LAUNCH_CHECK();
    if (target) {
        hipLaunchKernelGGL(mask_predict_finish_kernel, dim3(1), dim3(256), 0, st, row_loss, n * tiles, labels, n, c, hw,
                           valid_rows ? 1 : 0, loss, inv_div);
        IIF_LAUNCH_CHECK();
    }
    return IIF_OK;
}

int iif_normed_mask_predict_bwd_input(const void* x, int dtype, const float* g, const float* coef_a, const float* coef_b,
                                      const float* up, const float* inv_div, const float* weight, int64_t ld_w,
                                      const int64_t* labels, int n, int c, int cin, int hw, float power, float eps, void* dx,
                                      void* stream) {
    if (!geometry_ok(n, c, cin, hw) || ld_w < cin || !dtype_ok(dtype) || !(power > 0.f)) return IIF_EINVAL;
    if (!x || !g || !coef_a || !coef_b || !weight || !labels || !dx) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((cin + kChunk - 1) / kChunk, n);
    dispatch_row(dtype, wide_ok(x, dtype, hw) && wide_ok(dx, dtype, hw), [&](auto t, auto v) {
        using T = decltype(t);
        hipLaunchKernelGGL((normed_predict_dx_kernel<T, decltype(v)::value>), grid, dim3(256), 0, st, (const T*)x, g, coef_a, coef_b,
                           up, inv_div, weight, ld_w, labels, c, cin, hw, power, eps, (T*)dx);
    });
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_normed_mask_predict_bwd_weight(const void* x, int dtype, const float* g, const float* coef_a, const float* up,
                                       const float* inv_div, const float* weight, int64_t ld_w, const int64_t* labels, int n,
                                       int c, int cin, int hw, float power, float eps, float* scratch, float* dweight, float* dbias,
                                       void* stream) {
    if (!geometry_ok(n, c, cin, hw) || ld_w < cin || !dtype_ok(dtype) || !(power > 0.f)) return IIF_EINVAL;
    if (!x || !g || !coef_a || !weight || !labels || !scratch || (!dweight && !dbias)) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((cin + kChunk - 1) / kChunk, n);
    dispatch_row(dtype, wide_ok(x, dtype, hw), [&](auto t, auto v) {
        using T = decltype(t);
        hipLaunchKernelGGL((mask_predict_dw_rows_kernel<T, decltype(v)::value, true>), grid, dim3(256), 0, st, (const T*)x, g, coef_a,
                           up, inv_div, labels, c, cin, hw, 0, scratch);
    });
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(normed_predict_dw_classes_kernel, dim3(c), dim3(256), 0, st, scratch, labels, weight, ld_w, n, cin, power, eps,
                       dweight, dbias);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // extern "C"
