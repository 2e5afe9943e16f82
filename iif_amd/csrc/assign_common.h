// The pair arithmetic of the max-IoU assignment, shared by assign.hip (iif_max_iou_assign) and roi_stage.hip
// (iif_roi_stage_targets): one definition, so both produce the same bits.  Every step is the reference's single IEEE float32
// operation in its order (iou_calculators/iou2d_calculator.py:192-261, assigners/max_iou_assigner.py:141-183; the build passes
// -ffp-contract=off; `/` is the correctly rounded division).
#pragma once
#include "common.h"
#include "box_coder.h"

namespace {

constexpr float kAssignEps = 1e-6f;           // bbox_overlaps' default eps, which MaxIoUAssigner never overrides

__device__ __forceinline__ float box_area(const Box& b) { return (b.x2 - b.x1) * (b.y2 - b.y1); }

__device__ __forceinline__ float box_inter(const Box& a, const Box& b) {
    const float w = fmaxf(fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), 0.0f);
    const float h = fmaxf(fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1), 0.0f);
    return w * h;
}

// iou of a (ground-truth, candidate) pair as the assigner sees it (eps = kAssignEps > 0); `inter` returns the overlap area.
// BOTH passes go through this function: pass 2 compares its result with pass 1's for equality.
__device__ __forceinline__ float pair_iou(const Box& g, float ga, const Box& c, float ca, float& inter) {
    inter = box_inter(g, c);
    if (!(inter > 0.0f)) return 0.0f;                       // 0 / max(union, eps) = +0
    return inter / fmaxf(ga + ca - inter, kAssignEps);
}

__device__ __forceinline__ unsigned long long pack_max(float v, unsigned idx) {
    return ((unsigned long long)(__float_as_uint(v) + 1u) << 32) | (unsigned long long)(~idx);
}

// steps 1 - 3 of assign_wrt_overlaps (max_iou_assigner.py:141-183); A carries the thresholds pos, neg_lo, neg_hi
template <class A>
__device__ __forceinline__ int64_t base_assign(const A& a, float mo, int arg) {
    int64_t gi = -1;
    if (mo >= a.neg_lo && mo < a.neg_hi) gi = 0;
    if (mo >= a.pos) gi = (int64_t)arg + 1;
    return gi;
}

}  // namespace
