// Math the loss heads share: base-2 transcendentals on the hardware units (v_exp_f32 / v_log_f32, ~1 ulp) and the stable
// sigmoid element.
#pragma once
#include "common.h"

namespace {
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
__device__ __forceinline__ float fast_exp2(float v) { return __builtin_amdgcn_exp2f(v); }
__device__ __forceinline__ float fast_log2(float v) { return __builtin_amdgcn_logf(v); }
__device__ __forceinline__ float exp_neg(float v) { return __builtin_amdgcn_exp2f(-v * kLog2e); }   // e^-v

// softplus(x), softplus(-x), sigmoid(x) and 1 - sigmoid(x) of one logit.  With e = exp(-|x|), u = 1 + e, r = 1/u:
//   log1p(e) = ln(u) + (e - (u - 1)) * r        (u - 1 is exact: the bracket is u's rounding error, so small e keeps
//                                                 its digits without a polynomial or a second reciprocal)
//   sp(x) = max(x, 0) + log1p(e),  sp(-x) = max(-x, 0) + log1p(e)
//   s = sigmoid(x) = x >= 0 ? r : e*r,  q = 1 - s = x >= 0 ? e*r : r       (1 - s is never formed)
// Three transcendentals (v_exp_f32, v_rcp_f32, v_log_f32), and the exact function at every |x|: see DESIGN.md, "Sigmoid BCE /
// focal head".
struct SigmoidElem { float spp, spn, s, q; };

__device__ __forceinline__ SigmoidElem sigmoid_elem(float x) {
    const float e = exp_neg(fabsf(x));
    const float u = 1.0f + e;
    const float r = __builtin_amdgcn_rcpf(u);
    const float l1p = __builtin_amdgcn_logf(u) * kLn2 + (e - (u - 1.0f)) * r;
    const float er = e * r;
    SigmoidElem p;
    p.spp = fmaxf(x, 0.0f) + l1p;
    p.spn = fmaxf(-x, 0.0f) + l1p;
    p.s = x >= 0.0f ? r : er;
    p.q = x >= 0.0f ? er : r;
    return p;
}

// mmdet's binary_cross_entropy with one class index per row (cross_entropy_loss.py:53-111): the weighted loss l and d l / d x of
// the logit x in column c of a row whose target column is t (-1: a background row) and whose weight is wi (0 for an ignored
// row); pw is torch's pos_weight [C] or nullptr, read at the target column only.  bce_head.hip and head_loss.hip share it.
__device__ __forceinline__ void bce_label_elem(float x, int c, int t, float wi, const float* pw, float& l, float& d) {
    const SigmoidElem p = sigmoid_elem(x);
    l = p.spp;
    d = p.s;
    if (c == t) {
        const float w = pw ? pw[c] : 1.0f;
        l = w * p.spn;
        d = -w * p.q;
    }
    l *= wi;
    d *= wi;
}
}  // namespace
