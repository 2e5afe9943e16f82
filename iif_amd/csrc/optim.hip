// Fused RMSprop over a flat fp32 arena (classification/train.py:205-207: torch.optim.RMSprop with eps 0.0316, alpha 0.9).
// Per element, the arithmetic of torch's single-tensor RMSprop in the same order (torch/optim/rmsprop.py):
//   g   = grad_scale * grad;  g = g + wd * p                         (wd != 0)
//   sq  = alpha * sq + ((1 - alpha) * g) * g
//   CENTERED: ga = lerp(ga, g, 1 - alpha);  avg = sqrt(sq - ga * ga) + eps      else avg = sqrt(sq) + eps
//   MOMENTUM: buf = momentum * buf + g / avg;  p = p - lr * buf                 else p = p - lr * (g / avg)
// Correctly rounded sqrtf and IEEE division (no rsq / rcp, no fast-math; the library builds with -ffp-contract=off).
// Padding lanes of the arena (p = g = sq = buf = ga = 0) stay 0 as long as eps > 0: avg = eps there.
// Traffic per parameter: p, g, sq read + p, sq written = 20 B; + 8 B with MOMENTUM (buf), + 8 B with CENTERED (ga).
#include "common.h"
#include "stream_plan.h"

#include <math.h>

namespace {

using iif_plan::rms_blocks;    // stream_plan.h

template <bool MOMENTUM, bool CENTERED>
__device__ __forceinline__ void rmsprop_elem(float& p, float g, float& sq, float& buf, float& ga, float lr, float alpha,
                                             float one_m_alpha, float eps, float wd, float momentum, float grad_scale) {
    g = g * grad_scale;
    if (wd != 0.f) g = g + wd * p;
    sq = alpha * sq + (one_m_alpha * g) * g;
    float avg;
    if (CENTERED) {
        // torch.lerp: start + w * (end - start) for w < 0.5, end - (end - start) * (1 - w) otherwise
        const float d = g - ga;
        ga = one_m_alpha < 0.5f ? ga + one_m_alpha * d : g - d * (1.f - one_m_alpha);
        avg = sqrtf(sq - ga * ga) + eps;
    } else {
        avg = sqrtf(sq) + eps;
    }
    if (MOMENTUM) {
        buf = momentum * buf + g / avg;
        p = p - lr * buf;
    } else {
        p = p - lr * (g / avg);
    }
}

template <bool MOMENTUM, bool CENTERED>
__global__ void __launch_bounds__(256) rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq,
                                                      float* __restrict__ buf, float* __restrict__ ga, int64_t n, float lr,
                                                      const float* d_lr, float alpha, float eps, float wd, float momentum,
                                                      float grad_scale) {
    const float step = d_lr ? *d_lr : lr;
    const float one_m_alpha = 1.f - alpha;
    const int64_t n4 = n / 4;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 sv = reinterpret_cast<f32x4*>(sq)[i];
        f32x4 bv = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};
        if (MOMENTUM) bv = reinterpret_cast<f32x4*>(buf)[i];
        if (CENTERED) av = reinterpret_cast<f32x4*>(ga)[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float pq = pv[q], sq_ = sv[q], bq = bv[q], aq = av[q];
            rmsprop_elem<MOMENTUM, CENTERED>(pq, gv[q], sq_, bq, aq, step, alpha, one_m_alpha, eps, wd, momentum, grad_scale);
            pv[q] = pq; sv[q] = sq_; bv[q] = bq; av[q] = aq;
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(sq)[i] = sv;
        if (MOMENTUM) reinterpret_cast<f32x4*>(buf)[i] = bv;
        if (CENTERED) reinterpret_cast<f32x4*>(ga)[i] = av;
    }
    for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        float pq = p[i], sq_ = sq[i], bq = MOMENTUM ? buf[i] : 0.f, aq = CENTERED ? ga[i] : 0.f;
        rmsprop_elem<MOMENTUM, CENTERED>(pq, g[i], sq_, bq, aq, step, alpha, one_m_alpha, eps, wd, momentum, grad_scale);
        p[i] = pq;
        sq[i] = sq_;
        if (MOMENTUM) buf[i] = bq;
        if (CENTERED) ga[i] = aq;
    }
}

inline bool finite_nonneg(float v) { return v >= 0.f && v <= 3.402823466e38f; }   // false for NaN, -x and inf
inline bool mis16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

extern "C" int iif_rmsprop_step(float* params, const float* grads, float* square_avg, float* momentum_buf, float* grad_avg,
                                int64_t n, float lr, const float* d_lr, float alpha, float eps, float weight_decay,
                                float momentum, int centered, float grad_scale, void* stream) {
    if (n < 0) return IIF_EINVAL;
    if (!finite_nonneg(lr) || !finite_nonneg(eps) || !finite_nonneg(alpha) || !finite_nonneg(momentum) ||
        !finite_nonneg(weight_decay))
        return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    const bool mom = momentum > 0.f, cen = centered != 0;
    if (!params || !grads || !square_avg || (mom && !momentum_buf) || (cen && !grad_avg)) return IIF_EINVAL;
    if (mis16(params) || mis16(grads) || mis16(square_avg) || (mom && mis16(momentum_buf)) || (cen && mis16(grad_avg)))
        return IIF_EUNSUPPORTED;
    const dim3 grid(rms_blocks(n / 4 + 1)), block(256);
    hipStream_t st = as_stream(stream);
#define IIF_RMS_LAUNCH(M, C)                                                                                                    \
    hipLaunchKernelGGL((rmsprop_kernel<M, C>), grid, block, 0, st, params, grads, square_avg, M ? momentum_buf : nullptr,      \
                       C ? grad_avg : nullptr, n, lr, d_lr, alpha, eps, weight_decay, momentum, grad_scale)
    if (mom && cen) IIF_RMS_LAUNCH(true, true);
    else if (mom) IIF_RMS_LAUNCH(true, false);
    else if (cen) IIF_RMS_LAUNCH(false, true);
    else IIF_RMS_LAUNCH(false, false);
#undef IIF_RMS_LAUNCH
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}
