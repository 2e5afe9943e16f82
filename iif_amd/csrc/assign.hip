// Max-IoU box assignment and the 2-D overlap calculator for gfx950 (MI355X): mmdet's MaxIoUAssigner.assign and bbox_overlaps.
//
// instance_segmentation/mmdet/core/bbox/assigners/max_iou_assigner.py:61-213 materialises the [G, N] overlap matrix of
// iou_calculators/iou2d_calculator.py:75-261 (the file's own count: 9 G N floats of temporaries), takes its maxima along both
// axes, walks the G ground-truth boxes in a Python loop (two launches per box) and asks pos_inds.numel() of the host.  The
// result is three vectors of length N, and the only quantity that crosses candidates is one maximum per ground-truth box.  Here:
//
//   iif_bbox_overlaps    the stand-alone calculator: 'iou' / 'iof' / 'giou', pairwise [M, N] or aligned [N], one lane per output.
//   iif_max_iou_assign   no [G, N] array anywhere.  One lane per candidate box; the ground-truth (and ignore) boxes pass through
//                        LDS in chunks of kChunk, so any G works.
//     pass 1  (assign_pass1_chunks, assign_common.h) per candidate: is it ignored (max iof against the ignore boxes >
//             ignore_iof_thr), its maximum overlap and the LOWEST gt index that attains it.  Per gt: the maximum over the non-ignored candidates and the LOWEST candidate that
//             attains it, as a 64-bit INTEGER maximum of (bits(overlap) + 1) << 32 | ~candidate: an LDS atomic per overlapping
//             pair that beats the running LDS value, then one global atomic per gt and block that has one.  Overlaps are >= +0, so
//             their bits order as unsigned integers; 0 is "no candidate" (the reference's -1) and orders below bits(0.0) + 1.
//             Pairs that do not intersect (nearly all of them) issue nothing: their overlap is exactly +0, and what they contribute
//             to a gt's maximum - "0.0, at the lowest non-ignored candidate" - is ONE extra workspace slot for all gts.
//     pass 2  (match_low_quality only; without it pass 1 finishes the assignment in the same launch; step4_stage_chunk and
//             step4_hit, assign_common.h) applies the reference's steps in its order and recomputes the pairs it needs with the
//             same inline function, hence to the same bits: a candidate can only equal gt i's maximum if that maximum is <= the
//             candidate's own, which leaves few pairs.
//   Three enqueued operations at most: the workspace clear, pass 1, pass 2.  No float atomics: nothing depends on arrival order.
//
// Arithmetic: every step of the reference is one IEEE float32 operation, done here in its order (the build passes
// -ffp-contract=off; `/` is the correctly rounded division):
//     area = (x2 - x1) * (y2 - y1);  w, h = max(min(rb) - max(lt), 0);  overlap = w * h
//     union = max(area1 + area2 - overlap, eps)   ('iof': max(area1, eps));   iou = overlap / union
//     giou = iou - (max(enclose, eps) - union) / max(enclose, eps)
// The assigner's eps is the reference's default 1e-6 (> 0), so a pair with overlap == 0 has iou == +0 exactly and the division
// is skipped.  NaN coordinates are not reproduced (torch's max / clamp propagate NaN, v_max_f32 does not).
#include "common.h"
#include "assign_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = kAssignChunk;          // gt / ignore boxes per LDS chunk: one per thread of the block
static_assert(kThreads == kAssignChunk, "assign_pass1_chunks / step4_stage_chunk stage one box per thread");
constexpr unsigned kOvMaxBlocks = 1u << 16;   // grid cap of the calculator (grid-stride beyond)

enum { kIoU = 0, kIoF = 1, kGIoU = 2 };

struct AssignArgs {
    const float* b; int64_t ldb; int N; int vec_b;
    const float* g; int64_t ldg; int G;
    const float* ig; int64_t ldi; int I;                    // ig == nullptr: nothing is ignored
    float pos, neg_lo, neg_hi, min_pos, ign_thr;
    int assign_all, ign_wrt_cand, low_quality;
    const int64_t* gt_labels;
    int64_t* gt_inds; float* max_ov; int64_t* labels;
    u64* ws;                                                // [G + 1], zero on entry (low_quality only)
};

__device__ __forceinline__ void store_result(const AssignArgs& a, int64_t idx, int64_t gi) {
    a.gt_inds[idx] = gi;
    if (a.labels) a.labels[idx] = gi > 0 ? a.gt_labels[gi - 1] : (int64_t)-1;
}

__global__ void __launch_bounds__(kThreads) assign_pass1_kernel(AssignArgs a) {
    __shared__ Pass1Lds s;
    __shared__ unsigned s_low;                              // assign_pass1_chunks' slot
    const int tid = threadIdx.x;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + tid;
    const bool live = idx < a.N;
    if (a.G == 0) {                                         // no ground truth: everything is background (:146-162)
        if (live) {
            a.max_ov[idx] = 0.0f;
            store_result(a, idx, 0);
        }
        return;
    }
    Box c = {0.0f, 0.0f, 0.0f, 0.0f};
    float ca = 0.0f;
    if (live) {
        c = load_box(a.b + idx * a.ldb, a.vec_b != 0);
        ca = box_area(c);
    }

    // ---- ignored: max over the ignore boxes of iof > ignore_iof_thr (:108-118).  The threshold is > 0 here, so a pair that
    // does not intersect (iof = +0) never decides.
    bool ignored = false;
    if (a.ig) {
        for (int i0 = 0; i0 < a.I; i0 += kChunk) {
            const int cn = min(kChunk, a.I - i0);
            __syncthreads();
            if (tid < cn) {
                const Box q = load_box(a.ig + (int64_t)(i0 + tid) * a.ldi, false);
                s.box[tid] = q;
                s.area[tid] = box_area(q);
            }
            __syncthreads();
            if (live) {
                for (int j = 0; j < cn; ++j) {
                    const float inter = box_inter(c, s.box[j]);
                    if (inter > 0.0f) {
                        const float fg = a.ign_wrt_cand ? ca : s.area[j];
                        if (inter / fmaxf(fg, kAssignEps) > a.ign_thr) ignored = true;
                    }
                }
            }
        }
    }

    // ---- the candidate's maximum over the gts; the gts' maxima over the candidates that are not ignored
    float best = ignored ? -1.0f : 0.0f;                    // an ignored candidate has overlap -1 with every gt
    int arg = 0;
    const bool lq = a.low_quality != 0;
    assign_pass1_chunks(s, &s_low, a.g, a.ldg, a.G, c, ca, (unsigned)idx, live && !ignored, lq, a.ws, best, arg);
    if (live) {
        a.max_ov[idx] = best;
        if (lq) a.gt_inds[idx] = arg;                       // parked for pass 2
        else store_result(a, idx, base_assign(a, best, arg));
    }
}

// Step 4 (:185-200) on top of steps 1 - 3.  max_ov / gt_inds hold pass 1's per-candidate maximum and argmax.
__global__ void __launch_bounds__(kThreads) assign_pass2_kernel(AssignArgs a) {
    __shared__ Pass2Lds s;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = idx < a.N;
    float mo = 0.0f, ca = 0.0f;
    Box c = {0.0f, 0.0f, 0.0f, 0.0f};
    int64_t gi = -1;
    if (live) {
        mo = a.max_ov[idx];
        gi = base_assign(a, mo, (int)a.gt_inds[idx]);
        if (a.assign_all) {
            c = load_box(a.b + idx * a.ldb, a.vec_b != 0);
            ca = box_area(c);
        }
    }
    const bool ignored = mo == -1.0f;                       // overlaps are >= 0 otherwise
    const u64 zero_slot = a.ws[a.G];
    for (int g0 = 0; g0 < a.G; g0 += kChunk) {
        const int cn = min(kChunk, a.G - g0);
        step4_stage_chunk<false>(s, a.ws, zero_slot, a.min_pos, a.g, a.ldg, g0, cn, a.assign_all != 0);
        if (!live) continue;
        const int hit = step4_hit(s.box, s.area, s.gmax, s.garg, g0, cn, a.assign_all != 0, c, ca, mo, (int)idx, ignored);
        if (hit) gi = hit;
    }
    if (live) store_result(a, idx, gi);
}

struct OvArgs {
    const float* b1; int64_t ld1; int64_t m; int vec1;
    const float* b2; int64_t ld2; int64_t n; int vec2;
    float eps;
    float* out;
};

template <int MODE, bool ALIGNED>
__global__ void __launch_bounds__(kThreads) bbox_overlaps_kernel(OvArgs a) {
    const int64_t total = ALIGNED ? a.n : a.m * a.n;
    const int64_t step = (int64_t)gridDim.x * kThreads;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += step) {
        const int64_t i = ALIGNED ? e : e / a.n;
        const int64_t j = ALIGNED ? e : e - i * a.n;
        const Box p = load_box(a.b1 + i * a.ld1, a.vec1 != 0);
        const Box q = load_box(a.b2 + j * a.ld2, a.vec2 != 0);
        const float a1 = box_area(p);
        const float overlap = box_inter(p, q);
        float uni = MODE == kIoF ? a1 : a1 + box_area(q) - overlap;
        uni = fmaxf(uni, a.eps);
        float v = overlap / uni;
        if (MODE == kGIoU) {
            const float ew = fmaxf(fmaxf(p.x2, q.x2) - fminf(p.x1, q.x1), 0.0f);
            const float eh = fmaxf(fmaxf(p.y2, q.y2) - fminf(p.y1, q.y1), 0.0f);
            const float enc = fmaxf(ew * eh, a.eps);
            v = v - (enc - uni) / enc;
        }
        a.out[e] = v;
    }
}

template <int MODE, bool ALIGNED>
int launch_overlaps(const OvArgs& a, hipStream_t st) {
    const int64_t total = ALIGNED ? a.n : a.m * a.n;
    int64_t blocks = cdiv64(total, kThreads);
    blocks = blocks > kOvMaxBlocks ? kOvMaxBlocks : blocks;
    hipLaunchKernelGGL((bbox_overlaps_kernel<MODE, ALIGNED>), dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

bool f32_aligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }
bool rows_are_16_bytes(const void* p, int64_t ld) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 4 == 0; }

}  // namespace

extern "C" {

int iif_bbox_overlaps(const float* bboxes1, int64_t ld1, int64_t m, const float* bboxes2, int64_t ld2, int64_t n, int mode,
                      int aligned, float eps, float* out, void* stream) {
    if (m < 0 || n < 0 || m > INT32_MAX || n > INT32_MAX || ld1 < 4 || ld2 < 4) return IIF_EINVAL;
    if (mode != kIoU && mode != kIoF && mode != kGIoU) return IIF_EINVAL;
    if (aligned && m != n) return IIF_EINVAL;
    if (m == 0 || n == 0) return IIF_OK;
    if (!bboxes1 || !bboxes2 || !out) return IIF_EINVAL;
    if (!f32_aligned(bboxes1) || !f32_aligned(bboxes2) || !f32_aligned(out)) return IIF_EINVAL;
    OvArgs a{};
    a.b1 = bboxes1; a.ld1 = ld1; a.m = m; a.vec1 = rows_are_16_bytes(bboxes1, ld1);
    a.b2 = bboxes2; a.ld2 = ld2; a.n = n; a.vec2 = rows_are_16_bytes(bboxes2, ld2);
    a.eps = eps;
    a.out = out;
    hipStream_t st = as_stream(stream);
    if (aligned) {
        if (mode == kIoU) return launch_overlaps<kIoU, true>(a, st);
        if (mode == kIoF) return launch_overlaps<kIoF, true>(a, st);
        return launch_overlaps<kGIoU, true>(a, st);
    }
    if (mode == kIoU) return launch_overlaps<kIoU, false>(a, st);
    if (mode == kIoF) return launch_overlaps<kIoF, false>(a, st);
    return launch_overlaps<kGIoU, false>(a, st);
}

int iif_max_iou_assign(const float* bboxes, int64_t ld_bboxes, int64_t N, const float* gt_bboxes, int64_t ld_gt, int64_t G,
                       const float* ignore_bboxes, int64_t ld_ignore, int64_t I, float pos_iou_thr, float neg_lo, float neg_hi,
                       float min_pos_iou, float ignore_iof_thr, int gt_max_assign_all, int ignore_wrt_candidates,
                       int match_low_quality, const int64_t* gt_labels, int64_t* gt_inds, float* max_overlaps, int64_t* labels,
                       void* d_workspace, int64_t workspace_bytes, void* stream) {
    if (N < 0 || G < 0 || I < 0 || N > INT32_MAX || G >= INT32_MAX || I > INT32_MAX) return IIF_EINVAL;
    if (ld_bboxes < 4 || ld_gt < 4 || (ignore_bboxes && ld_ignore < 4)) return IIF_EINVAL;
    if (!(neg_lo <= neg_hi) || pos_iou_thr != pos_iou_thr || min_pos_iou != min_pos_iou) return IIF_EINVAL;
    if (!gt_inds || !max_overlaps) return IIF_EINVAL;
    if (labels && !gt_labels && G > 0) return IIF_EINVAL;
    if (N == 0) return IIF_OK;
    if (!bboxes || (G > 0 && !gt_bboxes)) return IIF_EINVAL;
    if (!f32_aligned(bboxes) || !f32_aligned(gt_bboxes) || !f32_aligned(ignore_bboxes) || !f32_aligned(max_overlaps)) return IIF_EINVAL;
    if (reinterpret_cast<uintptr_t>(gt_inds) % 8 != 0 || reinterpret_cast<uintptr_t>(labels) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(gt_labels) % 8 != 0)
        return IIF_EINVAL;
    const bool two_pass = match_low_quality && G > 0;
    if (two_pass) {
        if (!d_workspace || reinterpret_cast<uintptr_t>(d_workspace) % 8 != 0) return IIF_EINVAL;
        if (workspace_bytes < IIF_ASSIGN_WORKSPACE_BYTES(G)) return IIF_EINVAL;
    }
    AssignArgs a{};
    a.b = bboxes; a.ldb = ld_bboxes; a.N = (int)N; a.vec_b = rows_are_16_bytes(bboxes, ld_bboxes);
    a.g = gt_bboxes; a.ldg = ld_gt; a.G = (int)G;
    // the reference looks at the ignore boxes only for a threshold > 0 and a non-empty set (:108-109)
    const bool use_ignore = ignore_bboxes && I > 0 && ignore_iof_thr > 0.0f;
    a.ig = use_ignore ? ignore_bboxes : nullptr; a.ldi = ld_ignore; a.I = use_ignore ? (int)I : 0;
    a.pos = pos_iou_thr; a.neg_lo = neg_lo; a.neg_hi = neg_hi; a.min_pos = min_pos_iou; a.ign_thr = ignore_iof_thr;
    a.assign_all = gt_max_assign_all != 0; a.ign_wrt_cand = ignore_wrt_candidates != 0; a.low_quality = two_pass;
    a.gt_labels = gt_labels;
    a.gt_inds = gt_inds; a.max_ov = max_overlaps; a.labels = labels;
    a.ws = static_cast<u64*>(d_workspace);
    hipStream_t st = as_stream(stream);
    const unsigned blocks = (unsigned)cdiv64(N, kThreads);
    if (two_pass) {
        if (hipMemsetAsync(d_workspace, 0, (size_t)IIF_ASSIGN_WORKSPACE_BYTES(G), st) != hipSuccess) return IIF_ELAUNCH;
    }
    hipLaunchKernelGGL(assign_pass1_kernel, dim3(blocks), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    if (two_pass) {
        hipLaunchKernelGGL(assign_pass2_kernel, dim3(blocks), dim3(kThreads), 0, st, a);
        IIF_LAUNCH_CHECK();
    }
    return IIF_OK;
}

}  // extern "C"
