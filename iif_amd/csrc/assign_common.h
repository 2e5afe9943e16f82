// The max-IoU assignment, once: the pair arithmetic, the per-candidate / per-gt maxima of pass 1 and step 4 of pass 2, shared by
// assign.hip (iif_max_iou_assign), rpn_stage.hip (iif_rpn_stage_targets) and roi_stage.hip (iif_roi_stage_targets): one
// definition, so all three produce the same bits.  Every step is the reference's single IEEE float32 operation in its order
// (iou_calculators/iou2d_calculator.py:192-261, assigners/max_iou_assigner.py:141-183; the build passes -ffp-contract=off; `/`
// is the correctly rounded division).
#pragma once
#include "common.h"
#include "box_coder.h"

namespace {

typedef unsigned long long u64;

constexpr int kAssignChunk = 256;             // gt boxes per LDS chunk of the grid kernels: one per thread of their blocks
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

// A gt's maximum over the candidates and the LOWEST candidate that attains it, as one integer that orders like the pair:
// overlaps are >= +0, so their bits order as unsigned integers; 0 is "no candidate" and orders below bits(0.0) + 1.
__device__ __forceinline__ u64 pack_max(float v, unsigned idx) { return ((u64)(__float_as_uint(v) + 1u) << 32) | (u64)(~idx); }

template <int kScope>
__device__ __forceinline__ void fetch_max_guarded(u64* slot, u64 p) {
    if (p > __hip_atomic_load(slot, __ATOMIC_RELAXED, kScope)) __hip_atomic_fetch_max(slot, p, __ATOMIC_RELAXED, kScope);
}

// One (gt j, candidate i) pair of pass 1: the candidate's running maximum `best` at gt `arg` and, under low_quality, gt j's
// maximum in LDS.  A pair that does not intersect has overlap exactly +0 and issues nothing.
__device__ __forceinline__ void pair_update(const Box& g, float ga, int j, const Box& c, float ca, unsigned i, bool lq, u64* s_max_j,
                                            float& best, int& arg) {
    float inter;
    const float v = pair_iou(g, ga, c, ca, inter);
    if (inter > 0.0f) {
        if (v > best) { best = v; arg = j; }                // strict: ties stay with the lowest gt
        if (lq) fetch_max_guarded<__HIP_MEMORY_SCOPE_WORKGROUP>(s_max_j, pack_max(v, i));
    }
}

// Pass 1 of the grid kernels (blocks of kAssignChunk threads, G > 0), for candidate i with box c: the gts pass through LDS in
// chunks; `best` / `arg` come in as the candidate's start values and leave as its maximum and the lowest gt that attains it.
// Under low_quality each chunk's per-gt maxima go to ws[0 .. G) with one global atomic per gt and block that has one, and
// ws[G] gets pack_max(0.0, the lowest candidate that takes part): it holds every gt's maximum of 0.0 where no candidate
// intersects the gt.
//   part   whether the candidate takes part at all - the one thing the callers define differently: assign.hip `live and not
//          ignored` (an ignored candidate keeps its start value best = -1), rpn_stage.hip `takes_part(...)` on the image.
struct Pass1Lds { Box box[kAssignChunk]; float area[kAssignChunk]; u64 max[kAssignChunk]; };

__device__ __forceinline__ void assign_pass1_chunks(Pass1Lds& s, unsigned* s_low, const float* gt, int64_t ldg, int G, const Box& c, float ca,
                                                    unsigned i, bool part, bool lq, u64* ws, float& best, int& arg) {
    const int tid = threadIdx.x;
    if (tid == 0) *s_low = 0u;                              // ~(lowest candidate of the block that takes part), 0 = none
    for (int g0 = 0; g0 < G; g0 += kAssignChunk) {
        const int cn = min(kAssignChunk, G - g0);
        __syncthreads();
        if (tid < cn) {
            const Box q = load_box(gt + (int64_t)(g0 + tid) * ldg, false);
            s.box[tid] = q;
            s.area[tid] = box_area(q);
            s.max[tid] = 0ull;
        }
        __syncthreads();
        if (part)
            for (int j = 0; j < cn; ++j) pair_update(s.box[j], s.area[j], g0 + j, c, ca, i, lq, &s.max[j], best, arg);
        if (lq) {
            __syncthreads();
            if (tid < cn && s.max[tid] != 0ull) fetch_max_guarded<__HIP_MEMORY_SCOPE_AGENT>(ws + g0 + tid, s.max[tid]);
        }
    }
    if (lq) {
        const u64 m = __ballot(part);
        if (part && (threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1u)
            __hip_atomic_fetch_max(s_low, ~i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        if (tid == 0 && *s_low != 0u)                       // (1 << 32) | s_low = pack_max(0.0f, lowest)
            fetch_max_guarded<__HIP_MEMORY_SCOPE_AGENT>(ws + G, (1ull << 32) | (u64)*s_low);
    }
}

// steps 1 - 3 of assign_wrt_overlaps (max_iou_assigner.py:141-183); A carries the thresholds pos, neg_lo, neg_hi
template <class A>
__device__ __forceinline__ int64_t base_assign(const A& a, float mo, int arg) {
    int64_t gi = -1;
    if (mo >= a.neg_lo && mo < a.neg_hi) gi = 0;
    if (mo >= a.pos) gi = (int64_t)arg + 1;
    return gi;
}

// Step 4 (:185-200), the gt side: gt j's packed maximum `p` against `zero_slot` (what the non-intersecting pairs contribute:
// pack_max(0.0, lowest candidate that takes part), or 0 if none does) becomes gmax (NaN if gt j matches nothing) and garg (the
// candidate that attains it, -1 likewise).  A gt matches if its maximum is >= min_pos.
//   kEmptyInactive   what p == 0, "no candidate takes part", means.  false (assign.hip, roi_stage.hip): the reference's row is
//                    all -1, its maximum -1 at candidate 0, and min_pos decides as for any other.  true (rpn_stage.hip, whose
//                    reference compacted the candidates away): such a gt matches nothing.
// roi_stage.hip's zero_slot is the constant pack_max(0, 0) when it has a proposal: every proposal takes part.
template <bool kEmptyInactive>
__device__ __forceinline__ void decode_max(u64 p, u64 zero_slot, float min_pos, float& gmax, int& garg) {
    p = p > zero_slot ? p : zero_slot;
    const float gm = p ? __uint_as_float((unsigned)(p >> 32) - 1u) : -1.0f;
    const bool active = (!kEmptyInactive || p != 0ull) && gm >= min_pos;
    gmax = active ? gm : __uint_as_float(0x7fc00000u);
    garg = !active ? -1 : (p ? (int)~(unsigned)p : 0);
}

// One chunk of the gt side for the grid kernels: decode ws[g0 + tid] and, for assign_all, stage the gt box for step4_hit.
struct Pass2Lds { Box box[kAssignChunk]; float area[kAssignChunk]; float gmax[kAssignChunk]; int garg[kAssignChunk]; };

template <bool kEmptyInactive>
__device__ __forceinline__ void step4_stage_chunk(Pass2Lds& s, const u64* ws, u64 zero_slot, float min_pos, const float* gt,
                                                  int64_t ldg, int g0, int cn, bool assign_all) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < cn) {
        decode_max<kEmptyInactive>(ws[g0 + tid], zero_slot, min_pos, s.gmax[tid], s.garg[tid]);
        if (assign_all) {
            const Box q = load_box(gt + (int64_t)(g0 + tid) * ldg, false);
            s.box[tid] = q;
            s.area[tid] = box_area(q);
        }
    }
    __syncthreads();
}

// Step 4, the candidate side, over the gts g0 .. g0 + cn - 1 in LDS slots [0, cn): the new gt_inds (gt + 1) of candidate i for
// the highest gt that matches it, 0 if none (ascending, the last hit wins, as in the reference's loop).  gt_max_assign_all:
// every candidate whose overlap with gt j EQUALS gt j's maximum, the pair recomputed with pair_iou; a candidate can only equal
// it if it is <= the candidate's own maximum mo.  Otherwise: the one candidate garg[j].
//   ignored   assign.hip only: the candidate's overlap with every gt is -1 (mo = -1), so it equals a maximum of -1 without a
//             recomputation.  The other callers have no ignore boxes and pass false.
__device__ __forceinline__ int step4_hit(const Box* s_box, const float* s_area, const float* s_gmax, const int* s_garg, int g0, int cn,
                                         bool assign_all, const Box& c, float ca, float mo, int i, bool ignored) {
    int hit = 0;
    if (assign_all) {
        for (int j = 0; j < cn; ++j) {
            const float gm = s_gmax[j];
            if (!(gm <= mo)) continue;                      // overlap(j, this) <= mo < gm, or gt j takes no part
            float inter;
            if (ignored || pair_iou(s_box[j], s_area[j], c, ca, inter) == gm) hit = g0 + j + 1;
        }
    } else {
        for (int j = 0; j < cn; ++j)
            if (s_garg[j] == i) hit = g0 + j + 1;
    }
    return hit;
}

}  // namespace
