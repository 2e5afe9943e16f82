// Non-maximum suppression and the RPN proposal step for gfx950 (MI355X): mmcv's nms / batched_nms and mmdet's
// RPNHead.get_bboxes (instance_segmentation/mmdet/models/dense_heads/rpn_head.py:79-225) without a sort, a host copy of the
// suppression matrix or a host read.
//
//   iif_nms             5 enqueued operations for any N <= IIF_NMS_MAX_BOXES and any data:
//     clear     the 4 KiB workspace header (coordinate maximum, valid count).
//     prepare   one sort key per box: valid << 56 | order-preserving bits of the score << 24 | ~index; the ids as int32; the
//               maximum coordinate as an integer maximum of order-preserving bits.
//     rank      every box counts the keys greater than its own (keys stream through LDS in tiles of 1024, so N is not bounded
//               by LDS) and scatters itself to that position: score descending, equal scores to the lower index, boxes that
//               take no part behind all others.  With ids the ranked copy holds the SHIFTED coordinates box + id * (max + 1),
//               formed in float32 as batched_nms forms them.
//     matrix    the upper triangle of the suppression bit matrix in 64 x 64 tiles: one wave per tile, the column boxes in LDS,
//               one 64-bit word per (row, column block).  id_mode 2 tests pairs of equal id only.
//     scan      one workgroup: mmcv's greedy walk over the ranked list.  The 64 diagonal bits of a block-row are resolved in
//               one wave from registers (v_readlane); the words of the kept rows are ORed into a `removed` mask in LDS.  The
//               block-row r + 1 is loaded (all 64 rows, whatever will be decided) before block-row r is resolved, so the walk
//               never waits a memory round trip per kept box.  Writes keep, dets, the count and the padding; stops at max_num.
//   iif_rpn_proposals   10 enqueued operations for any B <= 16, any number of levels <= 8 and any data:
//     clear     header, histograms.
//     select    x 5: the nms_pre largest (logit, lower flattened index first) of every (image, level) at once: the radix select
//               of nms_common.h (select_pass_core) on the number logit bits << 24 | ~index.  No boundary pass, no ordered
//               sweep.  Scores and deltas are read in place through element strides.
//     gather    its sixth launch takes the elements at or above the threshold, decodes them with the coder's shared device function
//               (box_coder.h), computes the sigmoid, the min-size flag and the per-image coordinate maximum over the valid ones.
//               A candidate's slot within its level comes from an integer counter; the rank step orders them, so the
//               result does not depend on arrival order.
//     rank, matrix, scan   as above, for all images at once, with the level as id (id_mode 1) and the key built from the LOGIT
//               and the index into the concatenated anchors.
//
// The sort key, the overlap test (mmcv nms_cuda_kernel.cuh, each step one IEEE float32 operation, -ffp-contract=off), the
// counting rank and the 64-rank resolve of the scan are nms_common.h's.  Integer atomics only.  Nothing is allocated, nothing is read back.
#include "nms_common.h"
#include "box_coder.h"

namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;            // the scan: 256 word columns x 4 groups of 16 rows
constexpr int kMaxLevels = 8, kMaxImages = 16;
constexpr int kHeaderBytes = 4096;            // u32 words: [0, 16) coordinate maxima, [16, 144) level counters, [144, 160) valid counts
constexpr int kHdrCount = 16, kHdrValid = 144;
constexpr int64_t kHistBytes = (int64_t)kMaxLevels * kPasses * kBins * 4;     // per image
constexpr int64_t kFrontPerImage = kHistBytes + 4096;                          // ... and its selection states

static_assert(kFrontPerImage == 659456, "IIF_NMS_WORKSPACE_BYTES counts 659456 bytes of histograms and states per image");

// The sections of the workspace behind the header, histograms and states; Np = N rounded up to 64.
struct Ws {
    u32* hdr; u32* hist; SelState* state;
    u64* sk; f32x4* sbox; f32x4* cbox; int* sorig; int* sid; float* cscore; int* ccidx; int* clevel; u64* mask;
};

Ws carve(void* ws, int B, int64_t Np) {
    Ws w;
    char* p = static_cast<char*>(ws);
    w.hdr = reinterpret_cast<u32*>(p);
    w.hist = reinterpret_cast<u32*>(p + kHeaderBytes);
    w.state = reinterpret_cast<SelState*>(p + kHeaderBytes + (int64_t)B * kHistBytes);
    p += kHeaderBytes + (int64_t)B * kFrontPerImage;
    const int64_t e = (int64_t)B * Np;
    w.sk = reinterpret_cast<u64*>(p); p += 8 * e;
    w.sbox = reinterpret_cast<f32x4*>(p); p += 16 * e;
    w.cbox = reinterpret_cast<f32x4*>(p); p += 16 * e;
    w.sorig = reinterpret_cast<int*>(p); p += 4 * e;
    w.sid = reinterpret_cast<int*>(p); p += 4 * e;
    w.cscore = reinterpret_cast<float*>(p); p += 4 * e;
    w.ccidx = reinterpret_cast<int*>(p); p += 4 * e;
    w.clevel = reinterpret_cast<int*>(p); p += 4 * e;
    w.mask = reinterpret_cast<u64*>(p);
    return w;
}

// ------------------------------------------------------------------------------------------------ the NMS stage
struct NmsArgs {
    int B, N, Np, nw;
    const float* boxes; int64_t ldb, box_img;             // box i of image b: boxes + b * box_img + i * ldb
    const float* scores; int64_t score_img;
    const int* ids;                                       // [B][Np] int32 in the workspace, or nullptr
    int id_mode; float thr, offset;
    int64_t cap;
    int64_t* keep; float* dets; int64_t* count;
    Ws w;
    int64_t* cand_index; float* cand_boxes; float* cand_scores; int32_t* cand_level; int8_t* cand_valid;
};

struct PrepArgs {
    const float* boxes; int64_t ldb; const float* scores; const int64_t* ids; int N; float score_thr; int want_max;
    u64* sk; int* wid; u32* hdr;
};

__global__ void __launch_bounds__(kThreads) nms_prepare_kernel(PrepArgs a) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    u32 mk = 0u;
    if (i < a.N) {
        const float s = a.scores[i];
        const bool valid = !(a.score_thr > 0.0f) || s > a.score_thr;       // NMSop.forward: filters only for a threshold > 0
        a.sk[i] = sort_key(fkey(s), i, valid);
        if (a.ids) a.wid[i] = (int)a.ids[i];
        if (a.want_max) {
            const float* p = a.boxes + (int64_t)i * a.ldb;
            mk = box_max_key(p[0], p[1], p[2], p[3]);
        }
    }
    if (a.want_max) {
        mk = wave_max_u(mk);
        if ((threadIdx.x & 63) == 0 && mk != 0u) atomicMax(a.hdr, mk);
    }
}

__global__ void __launch_bounds__(kThreads) nms_rank_kernel(NmsArgs a) {
    __shared__ u64 s_tile[kRankTile];
    __shared__ int s_nv;
    const int tid = threadIdx.x, b = blockIdx.y;
    const int i = blockIdx.x * kThreads + tid;
    const int64_t row0 = (int64_t)b * a.Np;
    const u64* sk = a.w.sk + row0;
    const bool live = i < a.N;
    const u64 my = live ? sk[i] : 0ull;
    if (tid == 0) s_nv = 0;
    const int rank = count_greater_tiled<kThreads>(sk, a.N, my, s_tile);
    const bool valid = live && key_valid(my);
    const u64 vm = __ballot(valid);
    if ((tid & 63) == 0 && vm) atomicAdd(&s_nv, __popcll(vm));
    __syncthreads();
    if (tid == 0 && s_nv) atomicAdd(a.w.hdr + kHdrValid + b, (u32)s_nv);
    if (!live) return;
    const float* p = a.boxes + (int64_t)b * a.box_img + (int64_t)i * a.ldb;
    const Box box = {p[0], p[1], p[2], p[3]};
    const int id = a.ids ? a.ids[row0 + i] : 0;
    f32x4 s = {box.x1, box.y1, box.x2, box.y2};
    if (a.id_mode) {
        // batched_nms: offsets = idxs.to(boxes) * (boxes.max() + 1); boxes_for_nms = boxes + offsets[:, None]
        const float off = (float)id * (fkey_inv(a.w.hdr[b]) + 1.0f);
        s.x = box.x1 + off; s.y = box.y1 + off; s.z = box.x2 + off; s.w = box.y2 + off;
    }
    const int64_t o = row0 + rank;
    a.w.sbox[o] = s;
    a.w.sorig[o] = valid ? i : ~i;
    a.w.sid[o] = id;
    if (a.cand_index) {
        const int64_t c = (int64_t)b * a.N + rank;
        a.cand_index[c] = a.w.ccidx[row0 + i];
        if (a.cand_boxes) *reinterpret_cast<f32x4*>(a.cand_boxes + 4 * c) = f32x4{box.x1, box.y1, box.x2, box.y2};
        if (a.cand_scores) a.cand_scores[c] = a.scores[(int64_t)b * a.score_img + i];
        if (a.cand_level) a.cand_level[c] = id;
        if (a.cand_valid) a.cand_valid[c] = valid ? 1 : 0;
    }
}

// One wave per 64 x 64 tile of the upper triangle: lane = row, the 64 column boxes in LDS.
__global__ void __launch_bounds__(64) nms_matrix_kernel(NmsArgs a) {
    __shared__ f32x4 s_box[64];
    __shared__ float s_area[64];
    __shared__ int s_id[64];
    const int cb = blockIdx.x, rb = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    if (cb < rb) return;
    const int nv = (int)a.w.hdr[kHdrValid + b];
    if (rb * 64 >= nv) return;                               // rows that take no part are never read
    const int64_t row0 = (int64_t)b * a.Np;
    const float off = a.offset;
    const int j = cb * 64 + lane;
    if (j < nv) {
        const f32x4 q = a.w.sbox[row0 + j];
        s_box[lane] = q;
        s_area[lane] = nms_area(q, off);
        s_id[lane] = a.w.sid[row0 + j];
    }
    __syncthreads();
    const int i = rb * 64 + lane;
    if (i >= nv) return;
    const f32x4 p = a.w.sbox[row0 + i];
    const float sa = nms_area(p, off);
    const int id = a.w.sid[row0 + i];
    const bool same_id_only = a.id_mode == 2;
    const int cn = min(64, nv - cb * 64);
    u64 word = 0ull;
    for (int c = 0; c < cn; ++c) {
        const bool hit = nms_suppresses(p, sa, s_box[c], s_area[c], off, a.thr) && cb * 64 + c > i && (!same_id_only || s_id[c] == id);
        word |= hit ? (1ull << c) : 0ull;
    }
    a.w.mask[(row0 + i) * a.nw + cb] = word;
}

__global__ void __launch_bounds__(kScanThreads) nms_scan_kernel(NmsArgs a) {
    __shared__ u64 s_removed[256];
    __shared__ u64 s_kept;
    __shared__ int s_total;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int c = tid & 255, g = tid >> 8;                  // word column, group of 16 rows
    const int64_t row0 = (int64_t)b * a.Np;
    const int nw = a.nw;
    const u64* mask = a.w.mask + row0 * nw;
    int nv = (int)a.w.hdr[kHdrValid + b];
    nv = nv > a.N ? a.N : nv;
    const int nrb = (nv + 63) >> 6;
    const int64_t cap = a.cap;
    if (tid < 256) s_removed[tid] = 0ull;
    if (tid == 0) { s_total = 0; s_kept = 0ull; }

    // rows g * 16 .. + 15 of block-row r in column c (columns right of the diagonal), and the diagonal word of row `tid`
    u64 cur[16], nxt[16];
    u64 dcur = 0ull, dnxt = 0ull;
#pragma unroll
    for (int k = 0; k < 16; ++k) { cur[k] = 0ull; nxt[k] = 0ull; }
    if (nrb > 0) {
        if (c > 0 && c < nw) {
#pragma unroll
            for (int k = 0; k < 16; ++k) cur[k] = mask[(int64_t)(g * 16 + k) * nw + c];
        }
        if (tid < 64) dcur = mask[(int64_t)tid * nw];
    }
    int total = 0;
    for (int r = 0; r < nrb; ++r) {
        if (r + 1 < nrb) {
            const int64_t base = (int64_t)(r + 1) * 64;
            if (c > r + 1 && c < nw) {
#pragma unroll
                for (int k = 0; k < 16; ++k) nxt[k] = mask[(base + g * 16 + k) * nw + c];
            }
            if (tid < 64) dnxt = mask[(base + tid) * nw + r + 1];
        }
        __syncthreads();                                    // s_removed[r] is final
        if (tid < 64) {
            const int rows = min(64, nv - r * 64);
            const u64 kept = resolve_block64(dcur, s_removed[r] | (rows == 64 ? 0ull : ~0ull << rows), (int)(cap - total));
            if ((kept >> tid) & 1ull) {
                const int64_t pos = total + __popcll(kept & ((1ull << tid) - 1ull));
                const int o = a.w.sorig[row0 + r * 64 + tid];
                if (a.keep) a.keep[(int64_t)b * cap + pos] = o;
                if (a.dets) {
                    const float* p = a.boxes + (int64_t)b * a.box_img + (int64_t)o * a.ldb;
                    float* d = a.dets + ((int64_t)b * cap + pos) * 5;
                    d[0] = p[0]; d[1] = p[1]; d[2] = p[2]; d[3] = p[3];
                    d[4] = a.scores[(int64_t)b * a.score_img + o];
                }
            }
            if (tid == 0) { s_kept = kept; s_total = total + __popcll(kept); }
        }
        __syncthreads();
        const u64 kept = s_kept;
        total = s_total;
        if (total >= cap) break;                            // max_num: the rest of the walk cannot add a box
        if (c > r && c < nw) {
            const u32 kg = (u32)(kept >> (g * 16)) & 0xFFFFu;
            u64 acc = 0ull;
#pragma unroll
            for (int k = 0; k < 16; ++k) acc |= ((kg >> k) & 1u) ? cur[k] : 0ull;
            if (acc) atomicOr(&s_removed[c], acc);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) cur[k] = nxt[k];
        dcur = dnxt;
    }
    for (int64_t pos = total + tid; pos < cap; pos += kScanThreads) {
        if (a.keep) a.keep[(int64_t)b * cap + pos] = -1;
        if (a.dets) zero_det_row(a.dets + ((int64_t)b * cap + pos) * 5);
    }
    if (tid == 0) a.count[b] = total;
}

int launch_nms_stage(const NmsArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(nms_rank_kernel, dim3((unsigned)cdiv64(a.N, kThreads), (unsigned)a.B), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(nms_matrix_kernel, dim3((unsigned)a.nw, (unsigned)a.nw, (unsigned)a.B), dim3(64), 0, st, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(nms_scan_kernel, dim3((unsigned)a.B), dim3(kScanThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

// ------------------------------------------------------------------------------------------------ the RPN selection
struct RpnArgs {
    iif_rpn_level lv[kMaxLevels];
    int L, B, Np;
    int n[kMaxLevels], k[kMaxLevels], cand_off[kMaxLevels], anchor_off[kMaxLevels], vec_anchor[kMaxLevels];
    float max_h[kMaxImages], max_w[kMaxImages];
    Norm nm; float max_ratio, ctr_clamp, min_size; int add_ctr_clamp, clip;
    Ws w;
};

// select_pass_core's policy for segment (image b, level l): the number is logit bits << 24 | ~flattened index, read in place
// through the element strides; taking an element decodes it into the next slot of its level.
struct RpnSelect {
    struct Item { u64 number; float logit; int an, x, y; };
    static constexpr bool all = false;
    const RpnArgs& a; const iif_rpn_level& lv;
    int seg, b, l, n, k;
    u32* hist; SelState* state;
    u32 mk = 0u;                                            // the coordinate maximum over the valid boxes this thread took
    __device__ __forceinline__ RpnSelect(const RpnArgs& a_, int seg_)
        : a(a_), lv(a_.lv[seg_ % a_.L]), seg(seg_), b(seg_ / a_.L), l(seg_ % a_.L), hist(a_.w.hist), state(a_.w.state) {
        n = a.n[l]; k = a.k[l];
    }
    __device__ __forceinline__ Item load(int f) const {     // f = (h * W + w) * A + anchor
        Item it;
        it.an = f % lv.A;
        const int hw = f / lv.A;
        it.x = hw % lv.W; it.y = hw / lv.W;
        const float* sp = lv.scores + (int64_t)b * lv.score_strides[0];
        it.logit = sp[it.an * lv.score_strides[1] + it.y * lv.score_strides[2] + it.x * lv.score_strides[3]];
        it.number = sort_key(fkey(it.logit), f);
        return it;
    }
    __device__ __forceinline__ void take(int f, const Item& it) {
        const u32 slot = atomicAdd(a.w.hdr + kHdrCount + seg, 1u);
        if ((int)slot >= k) return;
        const Box anc = load_box(lv.anchors + (int64_t)f * lv.ld_anchors, a.vec_anchor[l] != 0);
        const float* d = lv.deltas + (int64_t)b * lv.delta_strides[0] + (int64_t)(4 * it.an) * lv.delta_strides[1] + it.y * lv.delta_strides[2] + it.x * lv.delta_strides[3];
        const Box t = {d[0], d[lv.delta_strides[1]], d[2 * lv.delta_strides[1]], d[3 * lv.delta_strides[1]]};
        const f32x4 o = decode_box(anc, t, a.nm, a.max_ratio, a.add_ctr_clamp, a.ctr_clamp, a.clip, a.max_h[b], a.max_w[b]);
        const bool valid = a.min_size < 0.0f || ((o.z - o.x) > a.min_size && (o.w - o.y) > a.min_size);
        const int cidx = a.anchor_off[l] + f;
        const int64_t at = (int64_t)b * a.Np + a.cand_off[l] + slot;
        a.w.cbox[at] = o;
        a.w.cscore[at] = 1.0f / (1.0f + expf(-it.logit));
        a.w.ccidx[at] = cidx;
        a.w.clevel[at] = l;
        a.w.sk[at] = sort_key((u32)(it.number >> 24), cidx, valid);
        if (valid) mk = max(mk, box_max_key(o.x, o.y, o.z, o.w));
    }
    __device__ __forceinline__ void finish() const {
        const u32 m = wave_max_u(mk);
        if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(a.w.hdr + b, m);
    }
};

__global__ void __launch_bounds__(kSelThreads) rpn_select_kernel(RpnArgs a, int p) {
    RpnSelect s(a, blockIdx.y);
    select_pass_core(s, p);
}

}  // namespace

extern "C" {

int iif_nms(const float* boxes, int64_t ld_boxes, const float* scores, const int64_t* ids, int64_t N, int id_mode,
            float iou_threshold, int offset, float score_threshold, int64_t max_num, int64_t* keep, float* dets, int64_t* count,
            void* d_workspace, int64_t workspace_bytes, void* stream) {
    if (N < 0 || N > IIF_NMS_MAX_BOXES || ld_boxes < 4 || id_mode < 0 || id_mode > 2 || (offset != 0 && offset != 1)) return IIF_EINVAL;
    if (iou_threshold != iou_threshold || score_threshold != score_threshold || !count || !aligned_to(count, 8)) return IIF_EINVAL;
    if (!aligned_to(boxes, 4) || !aligned_to(scores, 4) || !aligned_to(ids, 8) || !aligned_to(keep, 8) || !aligned_to(dets, 4)) return IIF_EINVAL;
    hipStream_t st = as_stream(stream);
    if (N == 0) {
        if (hipMemsetAsync(count, 0, 8, st) != hipSuccess) return IIF_ELAUNCH;
        return IIF_OK;
    }
    if (!boxes || !scores || !keep || (id_mode != 0 && !ids)) return IIF_EINVAL;
    if (!d_workspace || !aligned_to(d_workspace, 16) || workspace_bytes < IIF_NMS_WORKSPACE_BYTES(1, N)) return IIF_EINVAL;
    NmsArgs a{};
    a.B = 1; a.N = (int)N; a.Np = (int)((N + 63) / 64 * 64); a.nw = a.Np / 64;
    a.w = carve(d_workspace, 1, a.Np);
    a.boxes = boxes; a.ldb = ld_boxes; a.box_img = 0;
    a.scores = scores; a.score_img = 0;
    a.id_mode = id_mode; a.thr = iou_threshold; a.offset = (float)offset;
    a.cap = max_num > 0 && max_num < N ? max_num : N;
    a.keep = keep; a.dets = dets; a.count = count;
    // the unranked ids live in the candidate-level section, which the plain entry does not use otherwise
    a.ids = id_mode ? a.w.clevel : nullptr;
    PrepArgs p{};
    p.boxes = boxes; p.ldb = ld_boxes; p.scores = scores; p.ids = id_mode ? ids : nullptr; p.N = (int)N;
    p.score_thr = score_threshold; p.want_max = id_mode != 0;
    p.sk = a.w.sk; p.wid = a.w.clevel; p.hdr = a.w.hdr;
    if (hipMemsetAsync(d_workspace, 0, kHeaderBytes, st) != hipSuccess) return IIF_ELAUNCH;
    hipLaunchKernelGGL(nms_prepare_kernel, dim3((unsigned)cdiv64(N, kThreads)), dim3(kThreads), 0, st, p);
    IIF_LAUNCH_CHECK();
    return launch_nms_stage(a, st);
}

int iif_rpn_proposals(const iif_rpn_level* levels, int num_levels, int B, const float* img_hw, int nms_pre, int max_per_img,
                      float min_bbox_size, float iou_threshold, int offset, const float* means, const float* stds, float max_ratio,
                      int add_ctr_clamp, float ctr_clamp, int clip, float* dets, int64_t* counts, int64_t* cand_index,
                      float* cand_boxes, float* cand_scores, int32_t* cand_level, int8_t* cand_valid, void* d_workspace,
                      int64_t workspace_bytes, void* stream) {
    if (!levels || num_levels < 1 || num_levels > kMaxLevels || B < 1 || B > kMaxImages || !img_hw || !means || !stds) return IIF_EINVAL;
    if (max_per_img < 1 || (offset != 0 && offset != 1) || iou_threshold != iou_threshold || min_bbox_size != min_bbox_size) return IIF_EINVAL;
    if (!dets || !counts || !aligned_to(dets, 4) || !aligned_to(counts, 8) || !aligned_to(cand_index, 8) || !aligned_to(cand_boxes, 16) ||
        !aligned_to(cand_scores, 4) || !aligned_to(cand_level, 4))
        return IIF_EINVAL;
    if ((cand_boxes || cand_scores || cand_level || cand_valid) && !cand_index) return IIF_EINVAL;
    RpnArgs r{};
    int64_t ncand = 0, nanchor = 0;
    for (int l = 0; l < num_levels; ++l) {
        const iif_rpn_level& lv = levels[l];
        if (!lv.scores || !lv.deltas || !lv.anchors || !aligned_to(lv.scores, 4) || !aligned_to(lv.deltas, 4) || !aligned_to(lv.anchors, 4))
            return IIF_EINVAL;
        if (lv.A < 1 || lv.H < 1 || lv.W < 1 || lv.ld_anchors < 4) return IIF_EINVAL;
        const int64_t n = (int64_t)lv.A * lv.H * lv.W;
        if (n > (int64_t)kIndexMask) return IIF_EINVAL;
        const int64_t k = nms_pre > 0 && n > nms_pre ? nms_pre : n;
        r.lv[l] = lv;
        r.n[l] = (int)n; r.k[l] = (int)k; r.cand_off[l] = (int)ncand; r.anchor_off[l] = (int)nanchor;
        r.vec_anchor[l] = aligned_to(lv.anchors, 16) && lv.ld_anchors % 4 == 0;
        ncand += k; nanchor += n;
        if (ncand > IIF_NMS_MAX_BOXES || nanchor > (int64_t)kIndexMask) return IIF_EINVAL;
    }
    if (!d_workspace || !aligned_to(d_workspace, 16) || workspace_bytes < IIF_NMS_WORKSPACE_BYTES(B, ncand)) return IIF_EINVAL;
    const int Np = (int)((ncand + 63) / 64 * 64);
    r.L = num_levels; r.B = B; r.Np = Np;
    for (int b = 0; b < B; ++b) { r.max_h[b] = img_hw[2 * b]; r.max_w[b] = img_hw[2 * b + 1]; }
    for (int i = 0; i < 4; ++i) { r.nm.m[i] = means[i]; r.nm.s[i] = stds[i]; }
    r.max_ratio = max_ratio; r.ctr_clamp = ctr_clamp; r.min_size = min_bbox_size;
    r.add_ctr_clamp = add_ctr_clamp != 0; r.clip = clip != 0;
    r.w = carve(d_workspace, B, Np);
    NmsArgs a{};
    a.B = B; a.N = (int)ncand; a.Np = Np; a.nw = Np / 64;
    a.w = r.w;
    a.boxes = reinterpret_cast<const float*>(r.w.cbox); a.ldb = 4; a.box_img = 4 * (int64_t)Np;
    a.scores = r.w.cscore; a.score_img = Np;
    a.ids = r.w.clevel;
    a.id_mode = 1; a.thr = iou_threshold; a.offset = (float)offset;
    a.cap = max_per_img;
    a.keep = nullptr; a.dets = dets; a.count = counts;
    a.cand_index = cand_index; a.cand_boxes = cand_boxes; a.cand_scores = cand_scores; a.cand_level = cand_level; a.cand_valid = cand_valid;
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(d_workspace, 0, (size_t)(kHeaderBytes + (int64_t)B * kHistBytes), st) != hipSuccess) return IIF_ELAUNCH;
    for (int p = 0; p <= kPasses; ++p) {
        hipLaunchKernelGGL(rpn_select_kernel, dim3(kSelBlocks, (unsigned)(B * num_levels)), dim3(kSelThreads), 0, st, r, p);
        IIF_LAUNCH_CHECK();
    }
    return launch_nms_stage(a, st);
}

}  // extern "C"
