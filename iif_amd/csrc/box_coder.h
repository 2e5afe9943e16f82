// The box type and the two steps of the delta coder, shared by targets.hip (iif_bbox2delta / iif_delta2bbox, the target builders),
// nms.hip (the RPN proposals), assign.hip and roi_stage.hip: one definition, so all produce the same bits.  Every step is the
// reference's single IEEE float32 operation in its order (core/bbox/coder/delta_xywh_bbox_coder.py:119-139, :206-270; the build
// passes -ffp-contract=off); logf / expf are the device library's.
#pragma once
#include "common.h"

namespace {

struct alignas(16) Box { float x1, y1, x2, y2; };
struct Norm { float m[4], s[4]; };

// vec: the array's rows are whole 16-byte pieces (base on a 16-byte boundary, pitch a multiple of 4)
__device__ __forceinline__ Box load_box(const float* p, bool vec) {
    if (vec) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        return Box{t.x, t.y, t.z, t.w};
    }
    return Box{p[0], p[1], p[2], p[3]};
}

// torch.where(x < 0, 0, x) then torch.where(x > hi, hi, x): a NaN fails both comparisons and passes through
__device__ __forceinline__ float clip_coord(float x, float hi) {
    x = x < 0.0f ? 0.0f : x;
    return x > hi ? hi : x;
}
// torch.clamp: a NaN stays a NaN
__device__ __forceinline__ float clamp_lo(float x, float lo) { return x < lo ? lo : x; }
__device__ __forceinline__ float clamp_hi(float x, float hi) { return x > hi ? hi : x; }

// delta2bbox (:206-270) for one (box, delta) pair: p the anchor / roi, t the four deltas as (x1, y1, x2, y2) = (dx, dy, dw, dh)
__device__ __forceinline__ f32x4 decode_box(const Box& p, const Box& t, const Norm& nm, float max_ratio, int add_ctr_clamp,
                                            float ctr_clamp, int clip, float max_h, float max_w) {
    const float dx = t.x1 * nm.s[0] + nm.m[0];
    const float dy = t.y1 * nm.s[1] + nm.m[1];
    float dw = t.x2 * nm.s[2] + nm.m[2];
    float dh = t.y2 * nm.s[3] + nm.m[3];
    const float px = (p.x1 + p.x2) * 0.5f, py = (p.y1 + p.y2) * 0.5f;
    const float pw = p.x2 - p.x1, ph = p.y2 - p.y1;
    float dxw = pw * dx, dyh = ph * dy;
    if (add_ctr_clamp) {
        dxw = clamp_hi(clamp_lo(dxw, -ctr_clamp), ctr_clamp);
        dyh = clamp_hi(clamp_lo(dyh, -ctr_clamp), ctr_clamp);
        dw = clamp_hi(dw, max_ratio);
        dh = clamp_hi(dh, max_ratio);
    } else {
        dw = clamp_hi(clamp_lo(dw, -max_ratio), max_ratio);
        dh = clamp_hi(clamp_lo(dh, -max_ratio), max_ratio);
    }
    const float gw = pw * expf(dw), gh = ph * expf(dh);
    const float gx = px + dxw, gy = py + dyh;
    const float hw = gw * 0.5f, hh = gh * 0.5f;
    f32x4 o;
    o.x = gx - hw; o.y = gy - hh; o.z = gx + hw; o.w = gy + hh;
    if (clip) {
        o.x = clip_coord(o.x, max_w); o.y = clip_coord(o.y, max_h);
        o.z = clip_coord(o.z, max_w); o.w = clip_coord(o.w, max_h);
    }
    return o;
}

// bbox2delta (:119-139).  Shared by iif_bbox2delta, both target builders (targets.hip) and the RoI stage (roi_stage.hip).
__device__ __forceinline__ f32x4 encode_delta(const Box& p, const Box& g, const Norm& nm) {
    const float px = (p.x1 + p.x2) * 0.5f, py = (p.y1 + p.y2) * 0.5f;
    const float pw = p.x2 - p.x1, ph = p.y2 - p.y1;
    const float gx = (g.x1 + g.x2) * 0.5f, gy = (g.y1 + g.y2) * 0.5f;
    const float gw = g.x2 - g.x1, gh = g.y2 - g.y1;
    const float dx = (gx - px) / pw;
    const float dy = (gy - py) / ph;
    const float dw = logf(gw / pw);
    const float dh = logf(gh / ph);
    f32x4 o;
    o.x = (dx - nm.m[0]) / nm.s[0];
    o.y = (dy - nm.m[1]) / nm.s[1];
    o.z = (dw - nm.m[2]) / nm.s[2];
    o.w = (dh - nm.m[3]) / nm.s[3];
    return o;
}

}  // namespace
