// The training side of the RPN head for gfx950 (MI355X): anchors from a formula, targets for a whole batch without stored
// anchors, and the loss at the sampled anchors only.
//
// Mirror of core/anchor/anchor_generator.py:216-440 (grid_priors / grid_anchors / valid_flags), dense_heads/anchor_head.py:142-371
// (get_anchors, _get_targets_single, get_targets) and :373-491 with rpn_head.py's loss.
//
//   iif_grid_anchors / iif_grid_valid_flags   all levels in ONE launch each.  Anchor (l, y, x, a) is base[l][a] + (x sx, y sy, x sx,
//                        y sy): one float32 add per coordinate, the reference's.  The flag is x < vw and y < vh on integers.
//   iif_rpn_stage_targets   MaxIoUAssigner.assign on the anchors that are valid for the image, RandomSampler.sample and the encode
//                        of the sampled positives, for all B images (blockIdx.y), FIVE enqueued operations whatever B, the number of
//                        levels, G and the data:
//     clear    one hipMemsetAsync over the head of the workspace (per-gt maxima, key histograms, tickets).
//     pass 1   assign_pass1_chunks (assign_common.h), one lane per flat anchor index: the anchor is GENERATED from its index (base
//              anchors and level table arrive by value), the gts pass through LDS in chunks of 256, per-gt maxima are 64-bit
//              integer maxima of (bits(overlap) + 1) << 32 | ~index.  A candidate that is not valid for the image (valid_flags on
//              its pad_shape; anchor_inside_flags on its img_shape for allowed_border >= 0) takes no part at all: no maximum, not
//              the "lowest candidate" slot, later no class in the sampler.  The reference compacts these away; compaction is
//              monotone, so "lowest index wins" means the same in both index spaces.
//     pass 2   steps 1 - 4 in the reference's order (base_assign, step4_stage_chunk, step4_hit: assign_common.h) and the
//              histogram of the top 12 key bits per class (sample_core.h): LDS atomics, flushed with integer global atomics.
//     select   sample_select_core (sample_core.h) per image: budgets, threshold bins, one word per candidate; the last block of an
//              image (a ticket per image, no waiting) finds the threshold key, sweeps in index order, writes the ascending index
//              lists and - as the block that resolves the boundary - the encode of the positives it places.
//     total    num_total_samples = sum_b max(pos_b, 1) + max(neg_b, 1) as a float32 on the device.
//   Phases meet at launch boundaries only.  Integer atomics only: the same bits from call to call.
//   iif_rpn_stage_dense  the four dense per-level tensors of get_targets after images_to_levels, from the index lists: one lane
//                        per (image, anchor), a binary search in the two ascending lists, every element written once.
//   iif_rpn_loss_fwd     one launch, one workgroup per level: sum of w BCE_with_logits over the level's sampled anchors and of
//                        L1 / SmoothL1 over its positives, read IN PLACE from the NCHW / channels_last maps through
//                        (level, y, x, a); fixed summation order (strided per thread, shuffle tree, wave partials in order).
//   iif_rpn_loss_bwd     one launch: plain stores at the sampled positions of a gradient arena the caller cleared.
#include "common.h"
#include "assign_common.h"
#include "rpn_grid.h"
#include "sample_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = kAssignChunk;
static_assert(kThreads == kAssignChunk, "assign_pass1_chunks / step4_stage_chunk stage one box per thread");
constexpr int kPass2MaxBlocks = 512;
constexpr int kSelMaxBlocks = 64;

__device__ __forceinline__ Box make_anchor(const Grid& g, const Bases& bs, const Cell& c) {
    const float sx = (float)(c.x * g.lv[c.l].sx), sy = (float)(c.y * g.lv[c.l].sy);
    const float* b = bs.b[c.l][c.a];
    return Box{b[0] + sx, b[1] + sy, b[2] + sx, b[3] + sy};
}

// ------------------------------------------------------------------------------------------------ generator
struct GenArgs { Grid g; Bases bs; float* anchors; uint8_t* flags; int vw[kMaxLevels], vh[kMaxLevels]; };

__global__ void __launch_bounds__(kThreads) grid_anchors_kernel(GenArgs a) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.g.A) return;
    const Cell c = locate(a.g, i);
    const Box b = make_anchor(a.g, a.bs, c);
    f32x4 o;
    o.x = b.x1; o.y = b.y1; o.z = b.x2; o.w = b.y2;
    *reinterpret_cast<f32x4*>(a.anchors + 4 * (int64_t)i) = o;
}

__global__ void __launch_bounds__(kThreads) grid_flags_kernel(GenArgs a) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.g.A) return;
    const Cell c = locate(a.g, i);
    a.flags[i] = (uint8_t)(c.x < a.vw[c.l] && c.y < a.vh[c.l]);
}

// ------------------------------------------------------------------------------------------------ targets
struct Img { const float* gt; int64_t ldg; int G; int ws_off; float hi_w, hi_h; uint16_t vw[kMaxLevels], vh[kMaxLevels]; };

struct StageArgs {
    Grid g; Bases bs; Img im[kMaxImages];
    int As;                                                 // per-image pitch of the per-candidate arrays (A rounded up to 4)
    int use_border; float lo;
    const int32_t* keys;
    float pos, neg_lo, neg_hi, min_pos;
    int assign_all, low_quality;
    int nep, num; double ub; Norm nm;
    int64_t* pos_inds; int64_t* neg_inds; int64_t* counts; int64_t* pos_gt; float* pos_bt;
    u64* maxima; unsigned* hist; unsigned* tickets; float* mo; int* gi; unsigned* w;
};

__device__ __forceinline__ bool takes_part(const StageArgs& a, const Img& im, const Cell& c, const Box& b) {
    if (!(c.x < (int)im.vw[c.l] && c.y < (int)im.vh[c.l])) return false;
    if (a.use_border) return b.x1 >= a.lo && b.y1 >= a.lo && b.x2 < im.hi_w && b.y2 < im.hi_h;
    return true;
}

__global__ void __launch_bounds__(kThreads) rpn_pass1_kernel(StageArgs a) {
    __shared__ Pass1Lds s;
    __shared__ unsigned s_low;                              // assign_pass1_chunks' slot
    const int b = blockIdx.y;
    const Img& im = a.im[b];
    const int G = im.G;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < a.g.A;
    Box c = {0.0f, 0.0f, 0.0f, 0.0f};
    bool cand = false;
    if (live) {
        const Cell cell = locate(a.g, i);
        c = make_anchor(a.g, a.bs, cell);
        cand = takes_part(a, im, cell, c);
    }
    float* mo = a.mo + (int64_t)b * a.As;
    int* arg_out = a.gi + (int64_t)b * a.As;
    if (G == 0) {                                           // no ground truth: everything is background
        if (live) { mo[i] = 0.0f; arg_out[i] = cand ? 0 : -1; }
        return;
    }
    float best = 0.0f;
    int arg = 0;
    assign_pass1_chunks(s, &s_low, im.gt, im.ldg, G, c, box_area(c), (unsigned)i, cand, a.low_quality != 0, a.maxima + im.ws_off, best, arg);
    if (live) { mo[i] = best; arg_out[i] = cand ? arg : -1; }
}

// Steps 1 - 4 on pass 1's per-candidate maximum and argmax (the argmax slot becomes gt_inds: -1 takes no part, 0 negative,
// j + 1 gt j), and the histogram of the top 12 key bits per class.
__global__ void __launch_bounds__(kThreads) rpn_pass2_kernel(StageArgs a) {
    __shared__ Pass2Lds s;
    __shared__ unsigned s_hist[2 * kBins];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const Img& im = a.im[b];
    const int G = im.G;
    const float* mo_in = a.mo + (int64_t)b * a.As;
    int* gi_io = a.gi + (int64_t)b * a.As;
    const int32_t* keys = a.keys + (int64_t)b * a.g.A;
    const u64* ws = a.maxima + im.ws_off;
    const bool lq = a.low_quality != 0 && G > 0;
    hist_clear<kThreads>(s_hist);
    __syncthreads();
    const int tiles = (a.g.A + kThreads - 1) / kThreads;
    const u64 zero_slot = lq ? ws[G] : 0ull;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {          // uniform
        const int i = tile * kThreads + tid;
        const bool live = i < a.g.A;
        const int ar = live ? gi_io[i] : -1;
        const bool cand = ar >= 0;
        float mo = 0.0f, ca = 0.0f;
        Box c = {0.0f, 0.0f, 0.0f, 0.0f};
        int gi = -1;
        if (cand) {
            mo = mo_in[i];
            gi = G == 0 ? 0 : (int)base_assign(a, mo, ar);
            if (lq && a.assign_all) {
                c = make_anchor(a.g, a.bs, locate(a.g, i));
                ca = box_area(c);
            }
        }
        if (lq) {
            for (int g0 = 0; g0 < G; g0 += kChunk) {
                const int cn = min(kChunk, G - g0);
                step4_stage_chunk<true>(s, ws, zero_slot, a.min_pos, im.gt, im.ldg, g0, cn, a.assign_all != 0);
                if (!cand) continue;
                const int hit = step4_hit(s.box, s.area, s.gmax, s.garg, g0, cn, a.assign_all != 0, c, ca, mo, i, false);
                if (hit) gi = hit;
            }
        }
        if (live) {
            gi_io[i] = gi;
            if (gi >= 0) hist_add(s_hist, gi > 0 ? 0 : 1, sample_key(keys[i]));
        }
    }
    __syncthreads();
    hist_flush<kThreads>(s_hist, a.hist + (int64_t)b * 2 * kBins);
}

// sample_select_core's policy for image b: the class from pass 2's int gt_inds, no flags, and - as the block that resolves the
// boundary - the encode of each positive it places into pos_gt / pos_bt, zeros in their tails.
struct RpnSelect : SelectViews {
    static constexpr bool kFlags = false;
    const StageArgs& a; const Img& im; const int* gi; const int32_t* keys; int64_t row0;
    __device__ __forceinline__ RpnSelect(const StageArgs& a_, int b) : a(a_), im(a_.im[b]) {
        N = a.g.A; nep = a.nep; num = a.num; ub = a.ub;
        hist = a.hist + (int64_t)b * 2 * kBins; ticket = a.tickets + b; w = a.w + (int64_t)b * a.As;
        row0 = (int64_t)b * a.nep;
        pos_inds = a.pos_inds + row0; neg_inds = a.neg_inds + (int64_t)b * a.num; counts = a.counts + 2 * b;
        gi = a.gi + (int64_t)b * a.As; keys = a.keys + (int64_t)b * N;
    }
    __device__ __forceinline__ int cls(int64_t i) const { const int g = gi[i]; return g < 0 ? -1 : (g > 0 ? 0 : 1); }
    __device__ __forceinline__ unsigned key(int64_t i) const { return sample_key(keys[i]); }
    __device__ __forceinline__ void placed(unsigned slot, int64_t idx) const {
        int gt = gi[idx] - 1;
        gt = gt < 0 ? 0 : (gt >= im.G ? im.G - 1 : gt);                // a positive has 1 <= gt_inds <= G
        const Box anchor = make_anchor(a.g, a.bs, locate(a.g, (int)idx));
        const Box gb = load_box(im.gt + (int64_t)gt * im.ldg, false);
        a.pos_gt[row0 + slot] = gt;
        *reinterpret_cast<f32x4*>(a.pos_bt + 4 * (row0 + slot)) = encode_delta(anchor, gb, a.nm);
    }
    __device__ __forceinline__ void padded(int j) const {
        const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        a.pos_gt[row0 + j] = -1;
        *reinterpret_cast<f32x4*>(a.pos_bt + 4 * (row0 + j)) = z;
    }
};

__global__ void __launch_bounds__(kSelThreads) rpn_select_kernel(StageArgs a) { sample_select_core(RpnSelect(a, blockIdx.y)); }

__global__ void __launch_bounds__(64) rpn_total_kernel(const int64_t* counts, int B, float* out) {
    const int lane = threadIdx.x;
    int v = 0;
    if (lane < B) {
        const int64_t p = counts[2 * lane], n = counts[2 * lane + 1];
        v = (int)(p > 1 ? p : 1) + (int)(n > 1 ? n : 1);
    }
    v = wave_sum_i(v);
    if (lane == 0) *out = (float)v;
}

// ------------------------------------------------------------------------------------------------ the sampled lists, shared
// position of `i` in the ascending list[0 .. n), -1 if absent
__device__ __forceinline__ int find_in(const int64_t* list, int n, int64_t i) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < i) lo = mid + 1; else hi = mid;
    }
    return (lo < n && list[lo] == i) ? lo : -1;
}

struct DenseArgs {
    Grid g; Lists s; int64_t num_classes; float pos_weight;
    int64_t* labels; float* label_weights; float* bbox_targets; float* bbox_weights;
};

__global__ void __launch_bounds__(kThreads) rpn_dense_kernel(DenseArgs a) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= a.g.A) return;
    const int kp = clampi(a.s.counts[2 * b], a.s.nep), kn = clampi(a.s.counts[2 * b + 1], a.s.num);
    const Cell c = locate(a.g, i);
    const Lvl& v = a.g.lv[c.l];
    const int64_t Al = (int64_t)v.W * v.H * v.nb;
    const int64_t o = (int64_t)a.s.B * v.start + (int64_t)b * Al + c.r;
    int64_t label = a.num_classes;
    float lw = 0.0f;
    f32x4 bt = {0.0f, 0.0f, 0.0f, 0.0f}, bw = {0.0f, 0.0f, 0.0f, 0.0f};
    const int p = find_in(a.s.pos_inds + (int64_t)b * a.s.nep, kp, i);
    if (p >= 0) {
        label = 0;
        lw = a.pos_weight <= 0.0f ? 1.0f : a.pos_weight;
        bt = *reinterpret_cast<const f32x4*>(a.s.pos_bt + 4 * ((int64_t)b * a.s.nep + p));
        bw.x = bw.y = bw.z = bw.w = 1.0f;
    } else if (find_in(a.s.neg_inds + (int64_t)b * a.s.num, kn, i) >= 0) {
        lw = 1.0f;
    }
    a.labels[o] = label;
    a.label_weights[o] = lw;
    *reinterpret_cast<f32x4*>(a.bbox_targets + 4 * o) = bt;
    *reinterpret_cast<f32x4*>(a.bbox_weights + 4 * o) = bw;
}

// ------------------------------------------------------------------------------------------------ the loss
struct LossLvl { const float* scores; const float* deltas; float* g_scores; float* g_deltas; int64_t ss[4], ds[4], gss[4], gds[4]; };

struct LossArgs {
    Grid g; Lists s; LossLvl lv[kMaxLevels];
    const float* nts; float pos_weight, w_cls, w_box, beta;          // beta <= 0: L1
    float* out_cls; float* out_box;                                  // forward: [L] each
    const float* go_cls; const float* go_box;                        // backward: the gradients of those
};

__device__ __forceinline__ double block_sum_ordered(double v, double* s_w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < kSelThreads / 64; ++k) t += s_w[k];
    __syncthreads();
    return t;
}

__global__ void __launch_bounds__(kSelThreads) rpn_loss_fwd_kernel(LossArgs a) {
    __shared__ double s_w[kSelThreads / 64];
    const int l = blockIdx.x;
    const LossLvl& lv = a.lv[l];
    const int total = a.s.B * (a.s.nep + a.s.num);
    double cls = 0.0, box = 0.0;
    for (int e = threadIdx.x; e < total; e += kSelThreads) {
        int b, slot;
        bool pos;
        const int64_t idx = entry_of(a.s, e, b, pos, slot);
        if (idx < 0 || idx >= a.g.A) continue;
        const Cell c = locate(a.g, (int)idx);
        if (c.l != l) continue;
        const float x = lv.scores[b * lv.ss[0] + c.a * lv.ss[1] + c.y * lv.ss[2] + c.x * lv.ss[3]];
        const float t = pos ? 1.0f : 0.0f;
        const float bce = fmaxf(x, 0.0f) - x * t + log1pf(expf(-fabsf(x)));
        const float w = (pos && a.pos_weight > 0.0f) ? a.pos_weight : 1.0f;
        cls += (double)(w * bce);
        if (pos) {
            const float* tg = a.s.pos_bt + 4 * ((int64_t)b * a.s.nep + slot);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float p = lv.deltas[b * lv.ds[0] + (4 * c.a + j) * lv.ds[1] + c.y * lv.ds[2] + c.x * lv.ds[3]];
                const float d = fabsf(p - tg[j]);
                const float term = (a.beta > 0.0f && d < a.beta) ? 0.5f * d * d / a.beta : (a.beta > 0.0f ? d - 0.5f * a.beta : d);
                box += (double)term;
            }
        }
    }
    cls = block_sum_ordered(cls, s_w);
    box = block_sum_ordered(box, s_w);
    if (threadIdx.x == 0) {
        const float n = *a.nts;
        a.out_cls[l] = (float)cls / n * a.w_cls;
        a.out_box[l] = (float)box / n * a.w_box;
    }
}

__device__ __forceinline__ float sigmoidf_stable(float z) {
    if (z >= 0.0f) return 1.0f / (1.0f + expf(-z));
    const float e = expf(z);
    return e / (1.0f + e);
}

__global__ void __launch_bounds__(kThreads) rpn_loss_bwd_kernel(LossArgs a) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= a.s.B * (a.s.nep + a.s.num)) return;
    int b, slot;
    bool pos;
    const int64_t idx = entry_of(a.s, e, b, pos, slot);
    if (idx < 0 || idx >= a.g.A) return;
    const Cell c = locate(a.g, (int)idx);
    const LossLvl& lv = a.lv[c.l];
    const float n = *a.nts;
    const float x = lv.scores[b * lv.ss[0] + c.a * lv.ss[1] + c.y * lv.ss[2] + c.x * lv.ss[3]];
    const float w = (pos && a.pos_weight > 0.0f) ? a.pos_weight : 1.0f;
    const float dx = pos ? -sigmoidf_stable(-x) : sigmoidf_stable(x);          // sigmoid(x) - target, without the cancellation
    const float sc = a.go_cls[c.l] * a.w_cls / n;
    lv.g_scores[b * lv.gss[0] + c.a * lv.gss[1] + c.y * lv.gss[2] + c.x * lv.gss[3]] = sc * (w * dx);
    if (!pos) return;
    const float sb = a.go_box[c.l] * a.w_box / n;
    const float* tg = a.s.pos_bt + 4 * ((int64_t)b * a.s.nep + slot);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float p = lv.deltas[b * lv.ds[0] + (4 * c.a + j) * lv.ds[1] + c.y * lv.ds[2] + c.x * lv.ds[3]];
        const float d = p - tg[j];
        float gd = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
        if (a.beta > 0.0f && fabsf(d) < a.beta) gd = d / a.beta;
        lv.g_deltas[b * lv.gds[0] + (4 * c.a + j) * lv.gds[1] + c.y * lv.gds[2] + c.x * lv.gds[3]] = sb * gd;
    }
}

int64_t cleared_bytes(int B, int64_t total_G) {
    int64_t n = 8 * (total_G + B);
    n = (n + 15) / 16 * 16;                                 // the histograms are read in 16-byte pieces
    n += 4 * (int64_t)B * 2 * kBins + 4 * (int64_t)B;
    return (n + 15) / 16 * 16;
}

bool fill_loss(LossArgs* a, const iif_rpn_grid* grid, const iif_rpn_loss_level* levels, int B, bool backward) {
    if (!levels || !fill_grid(grid, &a->g, nullptr)) return false;
    for (int l = 0; l < a->g.L; ++l) {
        const iif_rpn_loss_level& m = levels[l];
        const bool empty = grid->W[l] == 0 || grid->H[l] == 0;
        if (!empty && (!m.scores || !m.deltas || (backward && (!m.grad_scores || !m.grad_deltas)))) return false;
        if (!aligned_to(m.scores, 4) || !aligned_to(m.deltas, 4) || !aligned_to(m.grad_scores, 4) || !aligned_to(m.grad_deltas, 4))
            return false;
        LossLvl& o = a->lv[l];
        o.scores = m.scores; o.deltas = m.deltas; o.g_scores = m.grad_scores; o.g_deltas = m.grad_deltas;
        for (int k = 0; k < 4; ++k) {
            if (m.score_strides[k] < 0 || m.delta_strides[k] < 0 || m.grad_score_strides[k] < 0 || m.grad_delta_strides[k] < 0) return false;
            o.ss[k] = m.score_strides[k]; o.ds[k] = m.delta_strides[k];
            o.gss[k] = m.grad_score_strides[k]; o.gds[k] = m.grad_delta_strides[k];
        }
    }
    return true;
}

}  // namespace

extern "C" {

int iif_grid_anchors(const iif_rpn_grid* grid, float* anchors, void* stream) {
    GenArgs a{};
    if (!fill_grid(grid, &a.g, &a.bs)) return IIF_EINVAL;
    if (a.g.A == 0) return IIF_OK;
    if (!anchors || !aligned_to(anchors, 16)) return IIF_EINVAL;
    a.anchors = anchors;
    hipLaunchKernelGGL(grid_anchors_kernel, dim3((unsigned)cdiv64(a.g.A, kThreads)), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_grid_valid_flags(const iif_rpn_grid* grid, const int32_t* valid_wh, uint8_t* flags, void* stream) {
    GenArgs a{};
    if (!fill_grid(grid, &a.g, nullptr) || !valid_wh) return IIF_EINVAL;
    for (int l = 0; l < a.g.L; ++l) {
        a.vw[l] = valid_wh[2 * l];
        a.vh[l] = valid_wh[2 * l + 1];
        if (a.vw[l] < 0 || a.vh[l] < 0) return IIF_EINVAL;
    }
    if (a.g.A == 0) return IIF_OK;
    if (!flags) return IIF_EINVAL;
    a.flags = flags;
    hipLaunchKernelGGL(grid_flags_kernel, dim3((unsigned)cdiv64(a.g.A, kThreads)), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int64_t iif_rpn_stage_workspace_bytes(int B, int64_t A, int64_t total_G) {
    if (B < 1 || B > kMaxImages || A < 0 || total_G < 0) return 0;
    const int64_t As = (A + 3) / 4 * 4;
    return cleared_bytes(B, total_G) + 3 * 4 * (int64_t)B * As;
}

int iif_rpn_stage_targets(const iif_rpn_grid* grid, const iif_roi_image* images, int B, const int32_t* valid_wh, int use_border,
                          float border_lo, const float* border_hi, const int32_t* keys, float pos_iou_thr, float neg_lo,
                          float neg_hi, float min_pos_iou, int gt_max_assign_all, int match_low_quality, int64_t num_expected_pos,
                          int64_t num, double neg_pos_ub, const float* means, const float* stds, int64_t* pos_inds,
                          int64_t* neg_inds, int64_t* counts, int64_t* pos_assigned_gt_inds, float* pos_bbox_targets,
                          float* num_total_samples, void* d_workspace, int64_t workspace_bytes, void* stream) {
    StageArgs a{};
    if (!fill_grid(grid, &a.g, &a.bs) || !images || !valid_wh || B < 1 || B > kMaxImages) return IIF_EINVAL;
    if (num < 0 || num > kMaxNum || num_expected_pos < 0 || num_expected_pos > num) return IIF_EINVAL;
    if (!(neg_lo <= neg_hi) || pos_iou_thr != pos_iou_thr || min_pos_iou != min_pos_iou || neg_pos_ub != neg_pos_ub) return IIF_EINVAL;
    if (!means || !stds || !counts || !num_total_samples || (use_border && !border_hi)) return IIF_EINVAL;
    if ((num_expected_pos > 0 && (!pos_inds || !pos_assigned_gt_inds || !pos_bbox_targets)) || (num > 0 && !neg_inds)) return IIF_EINVAL;
    if (a.g.A > 0 && !keys) return IIF_EINVAL;
    if (!aligned_to(keys, 4) || !aligned_to(pos_inds, 8) || !aligned_to(neg_inds, 8) || !aligned_to(counts, 8) ||
        !aligned_to(pos_assigned_gt_inds, 8) || !aligned_to(pos_bbox_targets, 16) || !aligned_to(num_total_samples, 4))
        return IIF_EINVAL;
    int64_t total_G = 0;
    for (int i = 0; i < B; ++i) {
        const iif_roi_image& m = images[i];
        if (m.G < 0) return IIF_EINVAL;
        if (m.G > 0 && (!m.gt_bboxes || m.ld_gt < 4 || !aligned_to(m.gt_bboxes, 4))) return IIF_EINVAL;
        Img& o = a.im[i];
        o.gt = m.gt_bboxes; o.ldg = m.ld_gt; o.G = m.G;
        if (total_G + i >= INT32_MAX) return IIF_EINVAL;
        o.ws_off = (int)(total_G + i);
        total_G += m.G;
        o.hi_w = use_border ? border_hi[2 * i] : 0.0f;
        o.hi_h = use_border ? border_hi[2 * i + 1] : 0.0f;
        for (int l = 0; l < a.g.L; ++l) {
            const int vw = valid_wh[(i * a.g.L + l) * 2], vh = valid_wh[(i * a.g.L + l) * 2 + 1];
            if (vw < 0 || vh < 0 || vw > 65535 || vh > 65535) return IIF_EINVAL;
            o.vw[l] = (uint16_t)vw; o.vh[l] = (uint16_t)vh;
        }
    }
    if (!d_workspace || !aligned_to(d_workspace, 16) || workspace_bytes < iif_rpn_stage_workspace_bytes(B, a.g.A, total_G))
        return IIF_EINVAL;
    const int64_t cleared = cleared_bytes(B, total_G);
    a.As = (a.g.A + 3) / 4 * 4;
    a.use_border = use_border != 0; a.lo = border_lo;
    a.keys = keys;
    a.pos = pos_iou_thr; a.neg_lo = neg_lo; a.neg_hi = neg_hi; a.min_pos = min_pos_iou;
    a.assign_all = gt_max_assign_all != 0; a.low_quality = match_low_quality != 0;
    a.nep = (int)num_expected_pos; a.num = (int)num; a.ub = neg_pos_ub;
    for (int i = 0; i < 4; ++i) { a.nm.m[i] = means[i]; a.nm.s[i] = stds[i]; }
    a.pos_inds = pos_inds; a.neg_inds = neg_inds; a.counts = counts; a.pos_gt = pos_assigned_gt_inds; a.pos_bt = pos_bbox_targets;
    char* ws = static_cast<char*>(d_workspace);
    a.maxima = reinterpret_cast<u64*>(ws);
    a.hist = reinterpret_cast<unsigned*>(ws + (8 * (total_G + B) + 15) / 16 * 16);
    a.tickets = a.hist + (int64_t)B * 2 * kBins;
    a.mo = reinterpret_cast<float*>(ws + cleared);
    a.gi = reinterpret_cast<int*>(a.mo + (int64_t)B * a.As);
    a.w = reinterpret_cast<unsigned*>(a.gi + (int64_t)B * a.As);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(d_workspace, 0, (size_t)cleared, st) != hipSuccess) return IIF_ELAUNCH;
    const int64_t tiles = a.g.A > 0 ? cdiv64(a.g.A, kThreads) : 1;
    hipLaunchKernelGGL(rpn_pass1_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(rpn_pass2_kernel, dim3((unsigned)(tiles > kPass2MaxBlocks ? kPass2MaxBlocks : tiles), (unsigned)B),
                       dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    int64_t sb = cdiv64(a.g.A, kSelThreads);
    sb = sb < 1 ? 1 : (sb > kSelMaxBlocks ? kSelMaxBlocks : sb);
    hipLaunchKernelGGL(rpn_select_kernel, dim3((unsigned)sb, (unsigned)B), dim3(kSelThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(rpn_total_kernel, dim3(1), dim3(64), 0, st, counts, B, num_total_samples);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_rpn_stage_dense(const iif_rpn_grid* grid, int B, const int64_t* pos_inds, const int64_t* neg_inds, const int64_t* counts,
                        const float* pos_bbox_targets, int64_t num_expected_pos, int64_t num, int64_t num_classes, float pos_weight,
                        int64_t* labels, float* label_weights, float* bbox_targets, float* bbox_weights, void* stream) {
    DenseArgs a{};
    if (!fill_grid(grid, &a.g, nullptr) || !fill_lists(&a.s, B, pos_inds, neg_inds, counts, pos_bbox_targets, num_expected_pos, num))
        return IIF_EINVAL;
    if (a.g.A == 0) return IIF_OK;
    if (!labels || !label_weights || !bbox_targets || !bbox_weights || !aligned_to(labels, 8) || !aligned_to(label_weights, 4) ||
        !aligned_to(bbox_targets, 16) || !aligned_to(bbox_weights, 16))
        return IIF_EINVAL;
    a.num_classes = num_classes; a.pos_weight = pos_weight;
    a.labels = labels; a.label_weights = label_weights; a.bbox_targets = bbox_targets; a.bbox_weights = bbox_weights;
    hipLaunchKernelGGL(rpn_dense_kernel, dim3((unsigned)cdiv64(a.g.A, kThreads), (unsigned)B), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_rpn_loss_fwd(const iif_rpn_grid* grid, const iif_rpn_loss_level* levels, int B, const int64_t* pos_inds,
                     const int64_t* neg_inds, const int64_t* counts, const float* pos_bbox_targets, int64_t num_expected_pos,
                     int64_t num, const float* num_total_samples, float pos_weight, float cls_loss_weight, float bbox_loss_weight,
                     float beta, float* loss_cls, float* loss_bbox, void* stream) {
    LossArgs a{};
    if (!fill_loss(&a, grid, levels, B, false) ||
        !fill_lists(&a.s, B, pos_inds, neg_inds, counts, pos_bbox_targets, num_expected_pos, num))
        return IIF_EINVAL;
    if (!num_total_samples || !loss_cls || !loss_bbox || !aligned_to(num_total_samples, 4) || !aligned_to(loss_cls, 4) ||
        !aligned_to(loss_bbox, 4))
        return IIF_EINVAL;
    a.nts = num_total_samples; a.pos_weight = pos_weight; a.w_cls = cls_loss_weight; a.w_box = bbox_loss_weight; a.beta = beta;
    a.out_cls = loss_cls; a.out_box = loss_bbox;
    hipLaunchKernelGGL(rpn_loss_fwd_kernel, dim3((unsigned)a.g.L), dim3(kSelThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_rpn_loss_bwd(const iif_rpn_grid* grid, const iif_rpn_loss_level* levels, int B, const int64_t* pos_inds,
                     const int64_t* neg_inds, const int64_t* counts, const float* pos_bbox_targets, int64_t num_expected_pos,
                     int64_t num, const float* num_total_samples, float pos_weight, float cls_loss_weight, float bbox_loss_weight,
                     float beta, const float* grad_loss_cls, const float* grad_loss_bbox, void* stream) {
    LossArgs a{};
    if (!fill_loss(&a, grid, levels, B, true) ||
        !fill_lists(&a.s, B, pos_inds, neg_inds, counts, pos_bbox_targets, num_expected_pos, num))
        return IIF_EINVAL;
    if (!num_total_samples || !grad_loss_cls || !grad_loss_bbox || !aligned_to(num_total_samples, 4) || !aligned_to(grad_loss_cls, 4) ||
        !aligned_to(grad_loss_bbox, 4))
        return IIF_EINVAL;
    a.nts = num_total_samples; a.pos_weight = pos_weight; a.w_cls = cls_loss_weight; a.w_box = bbox_loss_weight; a.beta = beta;
    a.go_cls = grad_loss_cls; a.go_box = grad_loss_bbox;
    const int64_t total = (int64_t)B * (a.s.nep + a.s.num);
    if (total == 0) return IIF_OK;
    hipLaunchKernelGGL(rpn_loss_bwd_kernel, dim3((unsigned)cdiv64(total, kThreads)), dim3(kThreads), 0, as_stream(stream), a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // extern "C"
