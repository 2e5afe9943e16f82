// Box sampling, the delta coder and the two target builders for gfx950 (MI355X): what lies between mmdet's assigner and its
// losses.
//
//   iif_bbox2delta / iif_delta2bbox   instance_segmentation/mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:98-272, one launch
//                        each (the reference: about twenty elementwise launches each).
//   iif_random_sample    core/bbox/samplers/base_sampler.py:35-102 + random_sampler.py:32-82 + the index lists of
//                        sampling_result.py, without nonzero / randperm / unique and without a host read.  The caller gives one
//                        random int32 key >= 0 per candidate; a class (positive: gt_inds > 0, negative: == 0) that has more
//                        members than its budget k keeps the k SMALLEST (key, index) pairs - equal keys go to the lower index.
//     clear   the 2 x 4096 counters and the ticket.
//     pass 1  (grid) histogram of the top 12 key bits per class: LDS atomics, flushed with integer global atomics.
//     pass 2  (grid) sample_select_core (sample_core.h, where the select is described) on the int64 gt_inds, with the flags:
//             budgets and threshold bins per block, one word per candidate, and the last block to finish (a ticket) resolves
//             the boundary bin and writes the ascending index lists.
//     Each of gt_inds and keys is read twice (pass 1, pass 2).  Integer atomics only: the result does not depend on arrival order.
//   iif_anchor_targets   dense_heads/anchor_head.py:224-265 with unmap_outputs: defaults, scatter, encode, unmap; one lane per
//                        anchor of the full set.
//   iif_roi_targets      roi_heads/bbox_heads/bbox_head.py:122-186 on the padded lists of iif_random_sample, with the gathers of
//                        sampling_result.py and bbox2roi: one lane per output row.
//
// Arithmetic of the coder: every step is the reference's single IEEE float32 operation in its order (the build passes
// -ffp-contract=off; `/` is the correctly rounded division); logf / expf are the device library's.
#include "common.h"
#include "box_coder.h"
#include "sample_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSampleMaxBlocks = 64;
constexpr int kTicketWord = 2 * kBins;        // workspace, in 32-bit words: [0, 8192) counters, [8192] ticket
constexpr int kWordsOffset = 65536 / 4;       // the per-candidate words start 64 KiB in
constexpr unsigned kMaxBlocks = 1u << 16;

struct EncArgs { const float* p; int64_t ldp; int vecp; const float* g; int64_t ldg; int vecg; int64_t n; Norm nm; float* out; };

__global__ void __launch_bounds__(kThreads) bbox2delta_kernel(EncArgs a) {
    const int64_t step = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += step) {
        const Box p = load_box(a.p + i * a.ldp, a.vecp != 0);
        const Box g = load_box(a.g + i * a.ldg, a.vecg != 0);
        *reinterpret_cast<f32x4*>(a.out + 4 * i) = encode_delta(p, g, a.nm);
    }
}

struct DecArgs {
    const float* r; int64_t ldr; int vecr; const float* d; int64_t ldd; int vecd; int64_t n; int K; Norm nm;
    float max_ratio, ctr_clamp, max_h, max_w; int add_ctr_clamp, clip;
    float* out;
};

// delta2bbox (:206-270), one lane per (row, class)
__global__ void __launch_bounds__(kThreads) delta2bbox_kernel(DecArgs a) {
    const int64_t total = a.n * a.K;
    const int64_t step = (int64_t)gridDim.x * kThreads;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += step) {
        const int64_t i = e / a.K;
        const int k = (int)(e - i * a.K);
        const Box p = load_box(a.r + i * a.ldr, a.vecr != 0);
        const Box t = load_box(a.d + i * a.ldd + 4 * k, a.vecd != 0);
        const f32x4 o = decode_box(p, t, a.nm, a.max_ratio, a.add_ctr_clamp, a.ctr_clamp, a.clip, a.max_h, a.max_w);
        *reinterpret_cast<f32x4*>(a.out + 4 * e) = o;
    }
}

// ------------------------------------------------------------------------------------------------ sampler
struct SampleArgs {
    const int64_t* gt_inds; const int32_t* keys; int N;
    int nep, num; double ub;
    int64_t* pos_inds; int64_t* neg_inds; int64_t* counts; int8_t* flags;
    unsigned* hist; unsigned* ticket; unsigned* w;
};

__global__ void __launch_bounds__(kSelThreads) sample_hist_kernel(SampleArgs a) {
    __shared__ unsigned h[2 * kBins];
    const int tid = threadIdx.x;
    hist_clear<kSelThreads>(h);
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * kSelThreads;
    for (int64_t i = (int64_t)blockIdx.x * kSelThreads + tid; i < a.N; i += step) {
        const int64_t gi = a.gt_inds[i];
        if (gi >= 0) hist_add(h, gi > 0 ? 0 : 1, sample_key(a.keys[i]));
    }
    __syncthreads();
    hist_flush<kSelThreads>(h, a.hist);
}

// sample_select_core's policy for one flat candidate set: the class from int64 gt_inds, the flags written, nothing else per positive
struct FlatSelect : SelectViews {
    static constexpr bool kFlags = true;
    const int64_t* gt_inds; const int32_t* keys; int8_t* flags;
    __device__ __forceinline__ int cls(int64_t i) const { const int64_t gi = gt_inds[i]; return gi < 0 ? -1 : (gi > 0 ? 0 : 1); }
    __device__ __forceinline__ unsigned key(int64_t i) const { return sample_key(keys[i]); }
    __device__ __forceinline__ void placed(unsigned, int64_t) const {}
    __device__ __forceinline__ void padded(int) const {}
};

__global__ void __launch_bounds__(kSelThreads) sample_select_kernel(SampleArgs a) {
    FlatSelect p;
    p.N = a.N; p.nep = a.nep; p.num = a.num; p.ub = a.ub;
    p.hist = a.hist; p.ticket = a.ticket; p.w = a.w;
    p.pos_inds = a.pos_inds; p.neg_inds = a.neg_inds; p.counts = a.counts;
    p.gt_inds = a.gt_inds; p.keys = a.keys; p.flags = a.flags;
    sample_select_core(p);
}

// ------------------------------------------------------------------------------------------------ target builders
struct AnchorArgs {
    const float* anchors; int64_t lda; int veca; int64_t A;
    const int8_t* flags; const int64_t* gt_inds; int64_t M;
    const float* gt; int64_t ldg; int64_t G; const int64_t* gt_labels; const int64_t* compact;
    int64_t background; float pos_weight; int decoded; Norm nm;
    int64_t* labels; float* label_weights; float* bbox_targets; float* bbox_weights;
};

__global__ void __launch_bounds__(kThreads) anchor_targets_kernel(AnchorArgs a) {
    const int64_t step = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.A; i += step) {
        int64_t label = a.background;
        float lw = 0.0f;
        f32x4 bt = {0.0f, 0.0f, 0.0f, 0.0f}, bw = {0.0f, 0.0f, 0.0f, 0.0f};
        const int64_t row = a.compact ? a.compact[i] : i;
        if (row >= 0 && row < a.M) {
            const int f = a.flags[row];
            if (f == 1) {
                const int64_t gi = a.gt_inds[row] - 1;
                if (gi >= 0 && gi < a.G) {
                    const Box g = load_box(a.gt + gi * a.ldg, false);
                    if (a.decoded) { bt.x = g.x1; bt.y = g.y1; bt.z = g.x2; bt.w = g.y2; }
                    else bt = encode_delta(load_box(a.anchors + i * a.lda, a.veca != 0), g, a.nm);
                    bw.x = bw.y = bw.z = bw.w = 1.0f;
                    label = a.gt_labels ? a.gt_labels[gi] : 0;
                    lw = a.pos_weight <= 0.0f ? 1.0f : a.pos_weight;
                }
            } else if (f == 2) {
                lw = 1.0f;
            }
        }
        a.labels[i] = label;
        a.label_weights[i] = lw;
        *reinterpret_cast<f32x4*>(a.bbox_targets + 4 * i) = bt;
        *reinterpret_cast<f32x4*>(a.bbox_weights + 4 * i) = bw;
    }
}

struct RoiArgs {
    const float* b; int64_t ldb; int vecb; int64_t N;
    const int64_t* gt_inds; const int64_t* labels_in; const float* gt; int64_t ldg; int64_t G;
    const int64_t* pos_inds; const int64_t* neg_inds; const int64_t* counts; int64_t cap, cap_pos;
    float img; int64_t num_classes; float pos_weight; int decoded; Norm nm;
    float* rois; int64_t* labels; float* label_weights; float* bbox_targets; float* bbox_weights; int64_t* pos_gt;
};

__global__ void __launch_bounds__(kThreads) roi_targets_kernel(RoiArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= a.cap) return;
    int64_t np = a.counts[0], nn = a.counts[1];
    np = np < 0 ? 0 : (np > a.cap_pos ? a.cap_pos : np);
    nn = nn < 0 ? 0 : (nn > a.cap ? a.cap : nn);
    int64_t label = a.num_classes, pg = -1;
    float lw = 0.0f;
    Box box = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 bt = {0.0f, 0.0f, 0.0f, 0.0f}, bw = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r < np + nn) {
        const bool pos = r < np;
        const int64_t idx = pos ? a.pos_inds[r] : a.neg_inds[r - np];
        if (idx >= 0 && idx < a.N) {
            box = load_box(a.b + idx * a.ldb, a.vecb != 0);
            lw = 1.0f;
            if (pos) {
                const int64_t gi = a.gt_inds[idx] - 1;
                if (gi >= 0 && gi < a.G) {
                    const Box g = load_box(a.gt + gi * a.ldg, false);
                    if (a.decoded) { bt.x = g.x1; bt.y = g.y1; bt.z = g.x2; bt.w = g.y2; }
                    else bt = encode_delta(box, g, a.nm);
                    bw.x = bw.y = bw.z = bw.w = 1.0f;
                    label = a.labels_in ? a.labels_in[idx] : 0;
                    lw = a.pos_weight <= 0.0f ? 1.0f : a.pos_weight;
                    pg = gi;
                }
            }
        }
    }
    float* ro = a.rois + 5 * r;
    ro[0] = a.img; ro[1] = box.x1; ro[2] = box.y1; ro[3] = box.x2; ro[4] = box.y2;
    a.labels[r] = label;
    a.label_weights[r] = lw;
    *reinterpret_cast<f32x4*>(a.bbox_targets + 4 * r) = bt;
    *reinterpret_cast<f32x4*>(a.bbox_weights + 4 * r) = bw;
    a.pos_gt[r] = pg;
}

bool rows_are_16_bytes(const void* p, int64_t ld) { return aligned_to(p, 16) && ld % 4 == 0; }

bool set_norm(Norm* nm, const float* means, const float* stds) {
    if (!means || !stds) return false;
    for (int i = 0; i < 4; ++i) { nm->m[i] = means[i]; nm->s[i] = stds[i]; }
    return true;
}

unsigned grid_for(int64_t n) {
    const int64_t b = cdiv64(n, kThreads);
    return (unsigned)(b > kMaxBlocks ? kMaxBlocks : b);
}

}  // namespace

extern "C" {

int iif_bbox2delta(const float* proposals, int64_t ld_proposals, const float* gt, int64_t ld_gt, int64_t n, const float* means,
                   const float* stds, float* out, void* stream) {
    EncArgs a{};
    if (n < 0 || n > INT32_MAX || ld_proposals < 4 || ld_gt < 4 || !set_norm(&a.nm, means, stds)) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    if (!proposals || !gt || !out || !aligned_to(proposals, 4) || !aligned_to(gt, 4) || !aligned_to(out, 16)) return IIF_EINVAL;
    a.p = proposals; a.ldp = ld_proposals; a.vecp = rows_are_16_bytes(proposals, ld_proposals);
    a.g = gt; a.ldg = ld_gt; a.vecg = rows_are_16_bytes(gt, ld_gt);
    a.n = n; a.out = out;
    hipLaunchKernelGGL(bbox2delta_kernel, dim3(grid_for(n)), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_delta2bbox(const float* rois, int64_t ld_rois, const float* deltas, int64_t ld_deltas, int64_t n, int num_classes,
                   const float* means, const float* stds, float max_ratio, int add_ctr_clamp, float ctr_clamp, int clip,
                   float max_h, float max_w, float* out, void* stream) {
    DecArgs a{};
    if (n < 0 || n > INT32_MAX || num_classes < 1 || ld_rois < 4 || ld_deltas < 4 * (int64_t)num_classes) return IIF_EINVAL;
    if (!set_norm(&a.nm, means, stds)) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    if (!rois || !deltas || !out || !aligned_to(rois, 4) || !aligned_to(deltas, 4) || !aligned_to(out, 16)) return IIF_EINVAL;
    a.r = rois; a.ldr = ld_rois; a.vecr = rows_are_16_bytes(rois, ld_rois);
    a.d = deltas; a.ldd = ld_deltas; a.vecd = rows_are_16_bytes(deltas, ld_deltas);
    a.n = n; a.K = num_classes;
    a.max_ratio = max_ratio; a.ctr_clamp = ctr_clamp; a.max_h = max_h; a.max_w = max_w;
    a.add_ctr_clamp = add_ctr_clamp != 0; a.clip = clip != 0;
    a.out = out;
    hipLaunchKernelGGL(delta2bbox_kernel, dim3(grid_for(n * num_classes)), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_random_sample(const int64_t* gt_inds, const int32_t* keys, int64_t N, int64_t num_expected_pos, int64_t num,
                      double neg_pos_ub, int64_t* pos_inds, int64_t* neg_inds, int64_t* counts, int8_t* flags, void* d_workspace,
                      int64_t workspace_bytes, void* stream) {
    if (N < 0 || N >= INT32_MAX - 4 || num < 0 || num > INT32_MAX || num_expected_pos < 0 || num_expected_pos > num) return IIF_EINVAL;
    if (neg_pos_ub != neg_pos_ub || !counts || (num_expected_pos > 0 && !pos_inds) || (num > 0 && !neg_inds)) return IIF_EINVAL;
    if (N > 0 && (!gt_inds || !keys || !flags)) return IIF_EINVAL;
    if (!aligned_to(gt_inds, 8) || !aligned_to(keys, 4) || !aligned_to(pos_inds, 8) || !aligned_to(neg_inds, 8) || !aligned_to(counts, 8))
        return IIF_EINVAL;
    if (!d_workspace || !aligned_to(d_workspace, 16) || workspace_bytes < IIF_SAMPLE_WORKSPACE_BYTES(N)) return IIF_EINVAL;
    SampleArgs a{};
    a.gt_inds = gt_inds; a.keys = keys; a.N = (int)N;
    a.nep = (int)num_expected_pos; a.num = (int)num; a.ub = neg_pos_ub;
    a.pos_inds = pos_inds; a.neg_inds = neg_inds; a.counts = counts; a.flags = flags;
    a.hist = static_cast<unsigned*>(d_workspace);
    a.ticket = a.hist + kTicketWord;
    a.w = a.hist + kWordsOffset;
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(d_workspace, 0, (size_t)(kTicketWord + 4) * 4, st) != hipSuccess) return IIF_ELAUNCH;
    int64_t blocks = cdiv64(N, kSelThreads);
    blocks = blocks < 1 ? 1 : (blocks > kSampleMaxBlocks ? kSampleMaxBlocks : blocks);
    if (N > 0) {
        hipLaunchKernelGGL(sample_hist_kernel, dim3((unsigned)blocks), dim3(kSelThreads), 0, st, a);
        IIF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sample_select_kernel, dim3((unsigned)blocks), dim3(kSelThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_anchor_targets(const float* anchors, int64_t ld_anchors, int64_t A, const int8_t* flags, const int64_t* gt_inds,
                       int64_t rows, const float* gt_bboxes, int64_t ld_gt, int64_t G, const int64_t* gt_labels,
                       const int64_t* compact_index, int64_t background_label, float pos_weight, int reg_decoded_bbox,
                       const float* means, const float* stds, int64_t* labels, float* label_weights, float* bbox_targets,
                       float* bbox_weights, void* stream) {
    AnchorArgs a{};
    if (A < 0 || A > INT32_MAX || rows < 0 || G < 0 || ld_anchors < 4 || ld_gt < 4 || !set_norm(&a.nm, means, stds)) return IIF_EINVAL;
    if (!compact_index && rows != A) return IIF_EINVAL;
    if (A == 0) return IIF_OK;
    if (!anchors || !labels || !label_weights || !bbox_targets || !bbox_weights) return IIF_EINVAL;
    if (rows > 0 && (!flags || !gt_inds)) return IIF_EINVAL;
    if (G > 0 && !gt_bboxes) return IIF_EINVAL;
    if (!aligned_to(anchors, 4) || !aligned_to(gt_bboxes, 4) || !aligned_to(gt_inds, 8) || !aligned_to(gt_labels, 8) ||
        !aligned_to(compact_index, 8) || !aligned_to(labels, 8) || !aligned_to(label_weights, 4) || !aligned_to(bbox_targets, 16) ||
        !aligned_to(bbox_weights, 16))
        return IIF_EINVAL;
    a.anchors = anchors; a.lda = ld_anchors; a.veca = rows_are_16_bytes(anchors, ld_anchors); a.A = A;
    a.flags = flags; a.gt_inds = gt_inds; a.M = rows;
    a.gt = gt_bboxes; a.ldg = ld_gt; a.G = G; a.gt_labels = gt_labels; a.compact = compact_index;
    a.background = background_label; a.pos_weight = pos_weight; a.decoded = reg_decoded_bbox != 0;
    a.labels = labels; a.label_weights = label_weights; a.bbox_targets = bbox_targets; a.bbox_weights = bbox_weights;
    hipLaunchKernelGGL(anchor_targets_kernel, dim3(grid_for(A)), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_roi_targets(const float* bboxes, int64_t ld_bboxes, int64_t N, const int64_t* gt_inds, const int64_t* labels_in,
                    const float* gt_bboxes, int64_t ld_gt, int64_t G, const int64_t* pos_inds, const int64_t* neg_inds,
                    const int64_t* counts, int64_t cap, int64_t cap_pos, int img_index, int64_t num_classes, float pos_weight,
                    int reg_decoded_bbox, const float* means, const float* stds, float* rois, int64_t* labels,
                    float* label_weights, float* bbox_targets, float* bbox_weights, int64_t* pos_assigned_gt_inds, void* stream) {
    RoiArgs a{};
    if (N < 0 || G < 0 || cap < 0 || cap > INT32_MAX || cap_pos < 0 || cap_pos > cap || ld_bboxes < 4 || ld_gt < 4) return IIF_EINVAL;
    if (!set_norm(&a.nm, means, stds)) return IIF_EINVAL;
    if (cap == 0) return IIF_OK;
    if (!counts || !neg_inds || (cap_pos > 0 && !pos_inds) || !rois || !labels || !label_weights || !bbox_targets || !bbox_weights ||
        !pos_assigned_gt_inds)
        return IIF_EINVAL;
    if (N > 0 && (!bboxes || !gt_inds)) return IIF_EINVAL;
    if (G > 0 && !gt_bboxes) return IIF_EINVAL;
    if (!aligned_to(bboxes, 4) || !aligned_to(gt_bboxes, 4) || !aligned_to(gt_inds, 8) || !aligned_to(labels_in, 8) ||
        !aligned_to(pos_inds, 8) || !aligned_to(neg_inds, 8) || !aligned_to(counts, 8) || !aligned_to(rois, 4) || !aligned_to(labels, 8) ||
        !aligned_to(label_weights, 4) || !aligned_to(bbox_targets, 16) || !aligned_to(bbox_weights, 16) ||
        !aligned_to(pos_assigned_gt_inds, 8))
        return IIF_EINVAL;
    a.b = bboxes; a.ldb = ld_bboxes; a.vecb = rows_are_16_bytes(bboxes, ld_bboxes); a.N = N;
    a.gt_inds = gt_inds; a.labels_in = labels_in; a.gt = gt_bboxes; a.ldg = ld_gt; a.G = G;
    a.pos_inds = pos_inds; a.neg_inds = neg_inds; a.counts = counts; a.cap = cap; a.cap_pos = cap_pos;
    a.img = (float)img_index; a.num_classes = num_classes; a.pos_weight = pos_weight; a.decoded = reg_decoded_bbox != 0;
    a.rois = rois; a.labels = labels; a.label_weights = label_weights; a.bbox_targets = bbox_targets; a.bbox_weights = bbox_weights;
    a.pos_gt = pos_assigned_gt_inds;
    hipLaunchKernelGGL(roi_targets_kernel, dim3((unsigned)cdiv64(cap, kThreads)), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // extern "C"
