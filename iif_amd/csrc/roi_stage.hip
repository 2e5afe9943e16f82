// The RoI head's training front end for gfx950 (MI355X), one workgroup per image, and the cascade's box refinement.
//
//   iif_roi_stage_targets   what StandardRoIHead.forward_train (roi_heads/standard_roi_head.py:85-100) and BBoxHead.get_targets
//                        (bbox_heads/bbox_head.py:188-261) do per image - MaxIoUAssigner.assign, add_gt_, RandomSampler.sample,
//                        _get_target_single, bbox2roi - for all images of a batch in ONE launch.  The number of valid proposals
//                        of each image is read from device memory, so the padded output of iif_rpn_proposals (or of
//                        iif_refine_bboxes below) feeds it without a host read.  A whole image (<= 4096 proposals, <= 1024
//                        ground-truth boxes) fits one workgroup: thread t owns the candidates t, t + 1024, ... (boxes, assignment
//                        and keys in registers), the ground-truth boxes and their maxima live in LDS.  No global workspace, no
//                        clear, no ticket.
//     assign   iif_max_iou_assign's definition (assign.hip's header comment) on the proposals alone, with the same inline
//              functions (assign_common.h: pair_update, decode_max, step4_hit over the LDS-resident ground truth): per-gt maxima
//              are 64-bit INTEGER maxima of (bits(overlap) + 1) << 32 | ~proposal in LDS.  Then the ground truth goes in front
//              as add_gt_ does: candidate c < G is gt c with gt_inds c + 1.
//     sample   iif_random_sample's rule and budgets (sample_core.h), by another route: a class with more members than its
//              budget keeps the k smallest (key, index) pairs.  The threshold key is found by a radix select over four digits of
//              the 31 key bits (LDS histograms); one ordered sweep (block scans, tile by tile in index order) then ranks the
//              members with exactly that key and gives every kept candidate its slot, so the lists are ascending.  Any keys
//              work, all equal included.
//     targets  the thread that owns a kept candidate writes its row: iif_roi_targets' rows, plus pos_is_gt and the
//              positives-only rows for the mask branch.
//   iif_refine_bboxes    BBoxHead.refine_bboxes + regress_by_class (bbox_head.py:380-496) on the padded rows of one stage: decode
//                        at the row's label, drop the rows that are ground truth, compact in order; the kept number stays on
//                        the device.
//
// Integer atomics only: no result depends on arrival order.
#include "common.h"
#include "assign_common.h"
#include "sample_core.h"

namespace {

constexpr int kThreads = kSelThreads;
static_assert(kThreads == 1024, "thread t owns the candidates t, t + 1024, ...; block_scan_excl is written for kSelThreads");
constexpr int kMaxImages = 16;
constexpr int kMaxProposals = 4096;
constexpr int kMaxGt = 1024;
constexpr int kMaxNum = 1024;
constexpr int kSlots = (kMaxProposals + kMaxGt) / kThreads;     // candidates per thread
constexpr int kDigits = 4;
constexpr int kDigitBins = 256;                                // per digit of the radix select (sample_core.h: kBins)

struct RoiImage { const float* gt; int64_t ldg; const int64_t* gt_labels; int G; float img; };

struct StageArgs {
    RoiImage im[kMaxImages];
    const float* props; int64_t ld_row, ld_img; int P; const int64_t* prop_counts;
    const int32_t* keys; int64_t ld_keys;
    float pos, neg_lo, neg_hi, min_pos;
    int assign_all, low_quality, add_gt;
    int nep, num; double ub;
    int64_t num_classes; float pos_weight; int decoded; Norm nm;
    float* rois; int64_t* labels; float* label_weights; float* bbox_targets; float* bbox_weights; int64_t* pos_gt;
    int64_t* counts; uint8_t* pos_is_gt; float* pos_rois; int64_t* pos_gt_inds; int64_t* pos_labels;
};

// digit d (0 = most significant) of a 31-bit key: 8, 8, 8 and 7 bits
__device__ __forceinline__ int digit_shift(int d) { return d == 0 ? 23 : (d == 1 ? 15 : (d == 2 ? 7 : 0)); }
__device__ __forceinline__ unsigned digit_of(unsigned key, int d) { return (key >> digit_shift(d)) & (d == 3 ? 127u : 255u); }
// the digits above d
__device__ __forceinline__ unsigned prefix_of(unsigned key, int d) { return d == 0 ? 0u : key >> (digit_shift(d - 1)); }

__global__ void __launch_bounds__(kThreads) roi_stage_kernel(StageArgs a) {
    __shared__ Box s_box[kMaxGt];
    __shared__ float s_area[kMaxGt];
    __shared__ u64 s_max[kMaxGt];
    __shared__ float s_gmax[kMaxGt];                        // the gt's maximum, NaN if it is below min_pos_iou (matches nothing)
    __shared__ int s_garg[kMaxGt];                          // the proposal that attains it, -1 likewise
    __shared__ unsigned s_hist[2 * kDigitBins];
    __shared__ u64 s_scan[kThreads / 64 + 1];
    __shared__ long long s_k[2], s_m[2];
    __shared__ unsigned s_prefix[2], s_rem[2];
    __shared__ int s_sel[2];                                // 1: the class needs the radix select

    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const RoiImage im = a.im[b];
    const int G = im.G;
    long long nb = a.P;
    if (a.prop_counts) {
        nb = a.prop_counts[b];
        nb = nb < 0 ? 0 : (nb > a.P ? a.P : nb);
    }
    const int n = (int)nb;
    const int front = (a.add_gt && G > 0) ? G : 0;          // ground-truth boxes in front of the proposals
    const int M = front + n;
    const float* props = a.props + (int64_t)b * a.ld_img;

    // ---- the ground truth into LDS
    for (int j = tid; j < G; j += kThreads) {
        const Box q = load_box(im.gt + (int64_t)j * im.ldg, false);
        s_box[j] = q;
        s_area[j] = box_area(q);
        s_max[j] = 0ull;
    }
    __syncthreads();

    // ---- this thread's candidates: c = tid + k * 1024; c < front is gt c, else proposal c - front
    Box bx[kSlots];
    float ca[kSlots], mo[kSlots];
    int arg[kSlots];
    int gi[kSlots];                                         // gt_inds: -1 ignored / nothing, 0 negative, i + 1 gt i
    const bool lq = a.low_quality != 0 && G > 0;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        const int c = tid + k * kThreads;
        bx[k] = Box{0.0f, 0.0f, 0.0f, 0.0f};
        ca[k] = 0.0f; mo[k] = 0.0f; arg[k] = 0; gi[k] = -1;
        if (c >= M) continue;
        if (c < front) {
            bx[k] = s_box[c];
            gi[k] = c + 1;
            continue;
        }
        const int i = c - front;
        bx[k] = load_box(props + (int64_t)i * a.ld_row, false);
        ca[k] = box_area(bx[k]);
        if (G == 0) { gi[k] = 0; continue; }                // no ground truth: everything is background (:146-162)
        float best = 0.0f;
        int ar = 0;
        for (int j = 0; j < G; ++j) pair_update(s_box[j], s_area[j], j, bx[k], ca[k], (unsigned)i, lq, &s_max[j], best, ar);
        mo[k] = best; arg[k] = ar;
        gi[k] = (int)base_assign(a, best, ar);
    }

    if (lq) {
        // Step 4 (:185-200).  Proposal 0 holds every gt's maximum of 0.0 where no proposal intersects the gt.
        __syncthreads();
        const u64 zero_slot = n > 0 ? pack_max(0.0f, 0u) : 0ull;
        for (int j = tid; j < G; j += kThreads) decode_max<false>(s_max[j], zero_slot, a.min_pos, s_gmax[j], s_garg[j]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSlots; ++k) {
            const int c = tid + k * kThreads;
            if (c >= M || c < front) continue;
            const int hit = step4_hit(s_box, s_area, s_gmax, s_garg, 0, G, a.assign_all != 0, bx[k], ca[k], mo[k], c - front, false);
            if (hit) gi[k] = hit;
        }
    }

    // ---- sampling: keys, class totals, budgets
    unsigned key[kSlots];
    int cls[kSlots];                                        // 0 positive, 1 negative, -1 takes no part
    for (int i = tid; i < 2 * kDigitBins; i += kThreads) s_hist[i] = 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        const int c = tid + k * kThreads;
        key[k] = 0u;
        cls[k] = -1;
        if (c < M && gi[k] >= 0) {
            cls[k] = gi[k] > 0 ? 0 : 1;
            key[k] = (unsigned)a.keys[(int64_t)b * a.ld_keys + c] & 0x7fffffffu;
            atomicAdd(&s_hist[cls[k] * kDigitBins + (int)digit_of(key[k], 0)], 1u);
        }
    }
    __syncthreads();
    if (tid == 0) {
        long long tot[2] = {0, 0};
        for (int i = 0; i < kDigitBins; ++i) { tot[0] += s_hist[i]; tot[1] += s_hist[kDigitBins + i]; }
        const Budgets bu = sample_budgets(tot[0], tot[1], a.nep, a.num, a.ub);
        s_k[0] = bu.kp; s_k[1] = bu.kn; s_m[0] = tot[0]; s_m[1] = tot[1];
    }
    __syncthreads();
    const long long kk[2] = {s_k[0], s_k[1]};
    if (tid < 2) {
        s_sel[tid] = kk[tid] > 0 && kk[tid] < s_m[tid];
        s_prefix[tid] = 0u;
        s_rem[tid] = (unsigned)(kk[tid] > 0 ? kk[tid] : 0);
    }
    __syncthreads();
    const int sel[2] = {s_sel[0], s_sel[1]};

    // ---- radix select: the k-th smallest key of a class, one digit at a time (digit 0's histogram is the one above)
    if (sel[0] || sel[1]) {
        for (int d = 0; d < kDigits; ++d) {
            if (d > 0) {
                for (int i = tid; i < 2 * kDigitBins; i += kThreads) s_hist[i] = 0u;
                __syncthreads();
                const unsigned pre[2] = {s_prefix[0], s_prefix[1]};
#pragma unroll
                for (int k = 0; k < kSlots; ++k)
                    if (cls[k] >= 0 && sel[cls[k]] && prefix_of(key[k], d) == pre[cls[k]])
                        atomicAdd(&s_hist[cls[k] * kDigitBins + (int)digit_of(key[k], d)], 1u);
                __syncthreads();
            }
            if (tid < 2 && sel[tid]) {
                const unsigned r = s_rem[tid];
                unsigned cum = 0u;
                const int bins = d == 3 ? 128 : kDigitBins;
                for (int i = 0; i < bins; ++i) {
                    const unsigned h = s_hist[tid * kDigitBins + i];
                    if (cum < r && r <= cum + h) {
                        s_prefix[tid] = (s_prefix[tid] << (d == 3 ? 7 : 8)) | (unsigned)i;
                        s_rem[tid] = r - cum;
                        break;
                    }
                    cum += h;
                }
            }
            __syncthreads();
        }
    }
    unsigned K[2], r3[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        // no select: everything of the class (every key is below 2^31) or nothing (no key is below 0, none equal is taken)
        K[c] = sel[c] ? s_prefix[c] : (kk[c] > 0 ? 0x80000000u : 0u);
        r3[c] = sel[c] ? s_rem[c] : 0u;
    }

    // ---- the ordered sweep and the rows
    const int64_t row0 = (int64_t)b * a.num, prow0 = (int64_t)b * a.nep;
    const int kp = (int)kk[0], kn = (int)kk[1];
    u64 run_eq = 0ull, run_sel = 0ull;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        if (k * kThreads >= M) break;                       // uniform
        const int c = tid + k * kThreads;
        int kind = 0;                                       // 0 not selected, 1 selected, 2 has the threshold key
        const int cl = cls[k];
        if (cl >= 0) {
            if (key[k] < K[cl]) kind = 1;
            else if (key[k] == K[cl]) kind = 2;
        }
        u64 tot;
        const u64 rank = block_scan_excl(kind == 2 ? one_of(cl) : 0ull, s_scan, &tot) + run_eq;
        run_eq += tot;
        if (kind == 2) kind = half_of(rank, cl) < r3[cl] ? 1 : 0;
        const u64 at = block_scan_excl(kind == 1 ? one_of(cl) : 0ull, s_scan, &tot) + run_sel;
        run_sel += tot;
        if (kind != 1) continue;
        const int slot = (int)half_of(at, cl);
        if (cl == 0 ? slot >= kp : slot >= kn) continue;    // cannot happen: the select takes exactly k
        const int r = cl == 0 ? slot : kp + slot;
        const Box box = bx[k];
        int64_t label = a.num_classes, pg = -1;
        float lw = 1.0f;
        f32x4 bt = {0.0f, 0.0f, 0.0f, 0.0f}, bw = {0.0f, 0.0f, 0.0f, 0.0f};
        if (cl == 0) {
            const int g = gi[k] - 1;
            const Box gb = s_box[g];
            if (a.decoded) { bt.x = gb.x1; bt.y = gb.y1; bt.z = gb.x2; bt.w = gb.y2; }
            else bt = encode_delta(box, gb, a.nm);
            bw.x = bw.y = bw.z = bw.w = 1.0f;
            label = im.gt_labels[g];
            lw = a.pos_weight <= 0.0f ? 1.0f : a.pos_weight;
            pg = g;
            float* pr = a.pos_rois + 5 * (prow0 + slot);
            pr[0] = im.img; pr[1] = box.x1; pr[2] = box.y1; pr[3] = box.x2; pr[4] = box.y2;
            a.pos_gt_inds[prow0 + slot] = g;
            a.pos_labels[prow0 + slot] = label;
        }
        const int64_t row = row0 + r;
        float* ro = a.rois + 5 * row;
        ro[0] = im.img; ro[1] = box.x1; ro[2] = box.y1; ro[3] = box.x2; ro[4] = box.y2;
        a.labels[row] = label;
        a.label_weights[row] = lw;
        *reinterpret_cast<f32x4*>(a.bbox_targets + 4 * row) = bt;
        *reinterpret_cast<f32x4*>(a.bbox_weights + 4 * row) = bw;
        a.pos_gt[row] = pg;
        a.pos_is_gt[row] = (uint8_t)(cl == 0 && c < front);
    }

    // ---- padding
    for (int r = kp + kn + tid; r < a.num; r += kThreads) {
        const int64_t row = row0 + r;
        float* ro = a.rois + 5 * row;
        ro[0] = im.img; ro[1] = 0.0f; ro[2] = 0.0f; ro[3] = 0.0f; ro[4] = 0.0f;
        a.labels[row] = a.num_classes;
        a.label_weights[row] = 0.0f;
        const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        *reinterpret_cast<f32x4*>(a.bbox_targets + 4 * row) = z;
        *reinterpret_cast<f32x4*>(a.bbox_weights + 4 * row) = z;
        a.pos_gt[row] = -1;
        a.pos_is_gt[row] = 0;
    }
    for (int s = kp + tid; s < a.nep; s += kThreads) {
        float* pr = a.pos_rois + 5 * (prow0 + s);
        pr[0] = -1.0f; pr[1] = 0.0f; pr[2] = 0.0f; pr[3] = 0.0f; pr[4] = 0.0f;
        a.pos_gt_inds[prow0 + s] = -1;
        a.pos_labels[prow0 + s] = a.num_classes;
    }
    if (tid == 0) {
        a.counts[2 * b] = kp;
        a.counts[2 * b + 1] = kn;
    }
}

struct RefineArgs {
    float hw[kMaxImages][2];
    const float* rois; int64_t ld_rois; const int64_t* labels; const float* preds; int64_t ld_preds; int C; int agnostic;
    const uint8_t* pos_is_gt; const int64_t* counts; int num;
    Norm nm; float max_ratio, ctr_clamp; int add_ctr_clamp, clip;
    float* out; int64_t* out_counts;
};

__global__ void __launch_bounds__(kThreads) refine_bboxes_kernel(RefineArgs a) {
    __shared__ u64 s_scan[kThreads / 64 + 1];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    long long valid = a.counts[2 * b] + a.counts[2 * b + 1];
    valid = valid < 0 ? 0 : (valid > a.num ? a.num : valid);
    const int64_t row0 = (int64_t)b * a.num;
    const float max_h = a.hw[b][0], max_w = a.hw[b][1];
    u64 run = 0ull;
    for (int t0 = 0; t0 < (int)valid; t0 += kThreads) {     // uniform
        const int r = t0 + tid;
        bool keep = false;
        f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
        if (r < valid && a.pos_is_gt[row0 + r] == 0) {
            keep = true;
            const int64_t row = row0 + r;
            const Box p = load_box(a.rois + row * a.ld_rois + 1, false);
            Box t = {0.0f, 0.0f, 0.0f, 0.0f};
            const int64_t lab = a.agnostic ? 0 : a.labels[row];
            if (lab >= 0 && lab < a.C) t = load_box(a.preds + row * a.ld_preds + 4 * lab, false);
            o = decode_box(p, t, a.nm, a.max_ratio, a.add_ctr_clamp, a.ctr_clamp, a.clip, max_h, max_w);
        }
        u64 tot;
        const u64 at = block_scan_excl(keep ? 1ull : 0ull, s_scan, &tot) + run;
        run += tot;
        if (keep) *reinterpret_cast<f32x4*>(a.out + 4 * (row0 + (int64_t)at)) = o;
    }
    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int r = (int)run + tid; r < a.num; r += kThreads) *reinterpret_cast<f32x4*>(a.out + 4 * (row0 + r)) = z;
    if (tid == 0) a.out_counts[b] = (int64_t)run;
}

}  // namespace

extern "C" {

int iif_roi_stage_targets(const iif_roi_image* images, int B, const float* proposals, int64_t ld_row, int64_t ld_image, int64_t P,
                          const int64_t* proposal_counts, const int32_t* keys, int64_t ld_keys, float pos_iou_thr, float neg_lo,
                          float neg_hi, float min_pos_iou, int gt_max_assign_all, int match_low_quality, int add_gt_as_proposals,
                          int64_t num_expected_pos, int64_t num, double neg_pos_ub, int64_t num_classes, float pos_weight,
                          int reg_decoded_bbox, const float* means, const float* stds, float* rois, int64_t* labels,
                          float* label_weights, float* bbox_targets, float* bbox_weights, int64_t* pos_assigned_gt_inds,
                          int64_t* counts, uint8_t* pos_is_gt, float* pos_rois, int64_t* pos_gt_inds, int64_t* pos_labels,
                          void* stream) {
    if (!images || B < 1 || B > kMaxImages || P < 0 || P > kMaxProposals || num < 0 || num > kMaxNum || num_expected_pos < 0 ||
        num_expected_pos > num)
        return IIF_EINVAL;
    if (ld_row < 4 || ld_image < 0 || (B > 1 && P > 0 && ld_image < 4)) return IIF_EINVAL;
    if (!(neg_lo <= neg_hi) || pos_iou_thr != pos_iou_thr || min_pos_iou != min_pos_iou || neg_pos_ub != neg_pos_ub) return IIF_EINVAL;
    if (!means || !stds || !counts) return IIF_EINVAL;
    if (P > 0 && !proposals) return IIF_EINVAL;
    if (num > 0 && (!rois || !labels || !label_weights || !bbox_targets || !bbox_weights || !pos_assigned_gt_inds || !pos_is_gt))
        return IIF_EINVAL;
    if (num_expected_pos > 0 && (!pos_rois || !pos_gt_inds || !pos_labels)) return IIF_EINVAL;
    if (!aligned_to(proposals, 4) || !aligned_to(proposal_counts, 8) || !aligned_to(keys, 4) || !aligned_to(rois, 4) ||
        !aligned_to(labels, 8) || !aligned_to(label_weights, 4) || !aligned_to(bbox_targets, 16) || !aligned_to(bbox_weights, 16) ||
        !aligned_to(pos_assigned_gt_inds, 8) || !aligned_to(counts, 8) || !aligned_to(pos_rois, 4) || !aligned_to(pos_gt_inds, 8) ||
        !aligned_to(pos_labels, 8))
        return IIF_EINVAL;
    StageArgs a{};
    int64_t max_front = 0;
    for (int i = 0; i < B; ++i) {
        const iif_roi_image& m = images[i];
        if (m.G < 0 || m.G > kMaxGt) return IIF_EINVAL;
        if (m.G > 0 && (!m.gt_bboxes || !m.gt_labels || m.ld_gt < 4 || !aligned_to(m.gt_bboxes, 4) || !aligned_to(m.gt_labels, 8)))
            return IIF_EINVAL;
        a.im[i].gt = m.gt_bboxes; a.im[i].ldg = m.ld_gt; a.im[i].gt_labels = m.gt_labels; a.im[i].G = m.G;
        a.im[i].img = (float)m.img_index;
        if (add_gt_as_proposals && m.G > max_front) max_front = m.G;
    }
    if (max_front + P > 0 && (!keys || ld_keys < max_front + P)) return IIF_EINVAL;
    a.props = proposals; a.ld_row = ld_row; a.ld_img = ld_image; a.P = (int)P; a.prop_counts = proposal_counts;
    a.keys = keys; a.ld_keys = ld_keys;
    a.pos = pos_iou_thr; a.neg_lo = neg_lo; a.neg_hi = neg_hi; a.min_pos = min_pos_iou;
    a.assign_all = gt_max_assign_all != 0; a.low_quality = match_low_quality != 0; a.add_gt = add_gt_as_proposals != 0;
    a.nep = (int)num_expected_pos; a.num = (int)num; a.ub = neg_pos_ub;
    a.num_classes = num_classes; a.pos_weight = pos_weight; a.decoded = reg_decoded_bbox != 0;
    for (int i = 0; i < 4; ++i) { a.nm.m[i] = means[i]; a.nm.s[i] = stds[i]; }
    a.rois = rois; a.labels = labels; a.label_weights = label_weights; a.bbox_targets = bbox_targets; a.bbox_weights = bbox_weights;
    a.pos_gt = pos_assigned_gt_inds; a.counts = counts; a.pos_is_gt = pos_is_gt;
    a.pos_rois = pos_rois; a.pos_gt_inds = pos_gt_inds; a.pos_labels = pos_labels;
    hipLaunchKernelGGL(roi_stage_kernel, dim3((unsigned)B), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_refine_bboxes(const float* rois, int64_t ld_rois, const int64_t* labels, const float* bbox_preds, int64_t ld_preds,
                      int num_classes, int reg_class_agnostic, const uint8_t* pos_is_gt, const int64_t* counts, int B, int64_t num,
                      const float* img_hw, const float* means, const float* stds, float max_ratio, int add_ctr_clamp,
                      float ctr_clamp, int clip, float* proposals, int64_t* proposal_counts, void* stream) {
    if (B < 1 || B > kMaxImages || num < 0 || num > kMaxNum || ld_rois < 5 || num_classes < 1) return IIF_EINVAL;
    if (ld_preds < 4 * (int64_t)(reg_class_agnostic ? 1 : num_classes)) return IIF_EINVAL;
    if (!means || !stds || !counts || !proposal_counts || (clip && !img_hw)) return IIF_EINVAL;
    if (num > 0 && (!rois || !bbox_preds || !pos_is_gt || !proposals || (!reg_class_agnostic && !labels))) return IIF_EINVAL;
    if (!aligned_to(rois, 4) || !aligned_to(labels, 8) || !aligned_to(bbox_preds, 4) || !aligned_to(counts, 8) ||
        !aligned_to(proposals, 16) || !aligned_to(proposal_counts, 8))
        return IIF_EINVAL;
    RefineArgs a{};
    for (int i = 0; i < B; ++i) {
        a.hw[i][0] = clip ? img_hw[2 * i] : 0.0f;
        a.hw[i][1] = clip ? img_hw[2 * i + 1] : 0.0f;
    }
    a.rois = rois; a.ld_rois = ld_rois; a.labels = labels; a.preds = bbox_preds; a.ld_preds = ld_preds;
    a.C = reg_class_agnostic ? 1 : num_classes; a.agnostic = reg_class_agnostic != 0;
    a.pos_is_gt = pos_is_gt; a.counts = counts; a.num = (int)num;
    for (int i = 0; i < 4; ++i) { a.nm.m[i] = means[i]; a.nm.s[i] = stds[i]; }
    a.max_ratio = max_ratio; a.ctr_clamp = ctr_clamp; a.add_ctr_clamp = add_ctr_clamp != 0; a.clip = clip != 0;
    a.out = proposals; a.out_counts = proposal_counts;
    hipLaunchKernelGGL(refine_bboxes_kernel, dim3((unsigned)B), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // extern "C"
