// mmdet's multiclass_nms (core/post_processing/bbox_nms.py:8-95, called from BBoxHead.get_bboxes) for gfx950 (MI355X): the
// score filter, mmcv's batched_nms in BOTH of its regimes and the final truncation, for B images at once, in 12 enqueued
// operations whatever the sizes and the data.  No sort, no N^2 matrix, nothing allocated, nothing read back.
//
// One image has R rows and C foreground classes; candidate (r, c) has the flat index f = r * C + c and takes part iff
// score[r, c] > score_thr (strict, on the raw score; rows at or beyond row_counts[b] never).  Its ranked score is
// score[r, c] * factor[r] when factors are given (one float32 multiply).  M = the number that takes part.  The sort key of a
// candidate is the one of nms.hip: order-preserving bits of the ranked score << 24 | ~f, so greater key = score descending,
// equal scores to the lower flat index, and all keys of an image are distinct.
//
//   clear      header (counters, maxima, selection states), histograms, class counters.
//   filter     one coalesced pass over the scores.  A candidate that takes part takes a slot in its class's segment (at most R
//              keys per class) through an integer counter, and a slot in the flat list through a counter that every workgroup
//              advances once (that counter ends as M).  The coordinate maximum over the boxes that take part is an integer maximum
//              of order-preserving bits.  Slots depend on arrival order; everything read from them is ranked first.
//   The regime is decided on the device: all pairs iff 0 < M < split_thr, else per class.  The kernels of the other regime
//   return at once.
//   flat rank  (all pairs)  every candidate of the flat list counts the keys greater than its own and scatters its key there.
//   flat walk  (all pairs)  one workgroup of 1024 threads per image walks the ranked list on the SHIFTED boxes
//              box + float(c) * (max + 1), formed in float32 as nms_rank_kernel forms them - boxes of different classes can
//              meet when coordinates lie below -1, as in mmcv.  Writes the kept keys in rank order; stops at cap.
//   class walk (per class)  one workgroup of 256 threads per (image, class): returns at once on an empty segment, else ranks
//              the segment's keys in LDS and walks them on the same shifted boxes.  Appends the kept keys to the image's kept
//              list through an integer counter.
//   select x 6 (per class)  the cap largest keys of the kept list: the radix select of nms_common.h (select_pass_core), one
//              segment per image.  With at most cap kept keys the histograms are skipped on the device.
//   finish     one workgroup per image ranks the at most cap selected keys in LDS and writes dets (the UNSHIFTED box and the
//              ranked score, recomputed from the inputs), labels, inds, the padding, counts and num_candidates.
//
// The walk (both regimes) holds no matrix.  Thread t keeps the shifted boxes of ranks t, t + T, ... in registers and one alive
// bit each.  Per block of 64 ranks: the owners publish their boxes to LDS; wave 0 tests the 64 x 64 pairs of the block itself
// (lane = row, one 64-bit word per lane) and resolves them in order with resolve_block64 (nms_common.h); then
// every thread tests its later boxes that are still alive against the boxes just kept.  Two barriers per 64 ranks (the LDS
// block is double-buffered), kept x m overlap tests in all, and the walk ends as soon as cap boxes are kept.  This is the
// only design that was measured (profiles/multiclass_nms.txt); the 128 KiB LDS bit matrix was not built.
//
// The sort key, both forms of the overlap test (-ffp-contract=off) and the counting ranks are nms_common.h's.  Integer atomics only.
#include "nms_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFilterItems = 8;               // candidates per thread of the filter
constexpr int kFlatCap = IIF_NMS_MAX_BOXES;   // all pairs: M < split_thr <= kFlatCap, or M <= R C <= kFlatCap
constexpr int kFlatThreads = 1024, kFlatPer = kFlatCap / kFlatThreads;
constexpr int kClassThreads = 256, kClassPer = IIF_MULTICLASS_NMS_MAX_ROWS / kClassThreads;
constexpr int kFinishThreads = 1024;
constexpr int kMaxImages = 16;
constexpr int kHeaderBytes = 4096;
// u32 words of the header, per image: coordinate maximum, M, kept keys, selected keys (all pairs), gather slots
constexpr int kHdrWords = 8, kHdrMax = 0, kHdrM = 1, kHdrKept = 2, kHdrSel = 3, kHdrSlot = 4;
constexpr int kStateOffset = 2048;            // SelState [B][kPasses] inside the header
constexpr int64_t kHistBytes = (int64_t)kPasses * kBins * 4;

static_assert(kMaxImages * kHdrWords * 4 <= kStateOffset && kStateOffset + kMaxImages * kPasses * 16 <= kHeaderBytes, "header layout");
static_assert(kHistBytes == 81920 && kFlatCap * 8 == 131072, "IIF_MULTICLASS_NMS_WORKSPACE_BYTES counts these");
static_assert(kClassPer * kClassThreads == IIF_MULTICLASS_NMS_MAX_ROWS && kFlatPer * kFlatThreads == kFlatCap, "walk capacity");

struct McArgs {
    int B, R, C, cap, n, split;               // n = R C; split: all pairs iff 0 < M < split
    const float* boxes; int64_t ldb; int per_class;
    const float* scores; int64_t lds;
    const float* factors; const int64_t* row_counts;
    float score_thr, thr, offset;
    float* dets; int64_t* labels; int64_t* inds; int64_t* counts; int64_t* ncand;
    u32* hdr; SelState* state; u32* hist; u32* ccnt; int ccnt_ld;
    u64* seg;                                 // [B][C][R]
    u64* list;                                // [B][n]: the flat list (all pairs) or the kept keys (per class)
    u64* ranked;                              // [B][kFlatCap]
    u64* sel;                                 // [B][cap]
};

__device__ __forceinline__ bool all_pairs(int M, int split) { return M > 0 && M < split; }

__device__ __forceinline__ const float* box_of(const McArgs& a, int b, int r, int c) {
    return a.boxes + ((int64_t)b * a.R + r) * a.ldb + (a.per_class ? 4 * c : 0);
}

__device__ __forceinline__ float ranked_score(const McArgs& a, int b, int r, int c) {
    const float s = a.scores[((int64_t)b * a.R + r) * a.lds + c];
    return a.factors ? s * a.factors[(int64_t)b * a.R + r] : s;
}

__global__ void __launch_bounds__(kThreads) mc_filter_kernel(McArgs a) {
    __shared__ u32 s_cnt[kFilterItems * (kThreads / 64)];
    __shared__ u32 s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
    u32* hdr = a.hdr + b * kHdrWords;
    int rows = a.R;
    if (a.row_counts) {
        const int64_t rc = a.row_counts[b];
        rows = rc < 0 ? 0 : (rc < a.R ? (int)rc : a.R);
    }
    u32 mk = 0u, valid = 0u;
    u64 key[kFilterItems];
    u32 before[kFilterItems];                 // valid candidates of this wave and item in lower lanes
#pragma unroll
    for (int k = 0; k < kFilterItems; ++k) {
        const int f = (blockIdx.x * kFilterItems + k) * kThreads + tid;
        bool v = false;
        key[k] = 0ull;
        if (f < a.n) {
            const int r = f / a.C, c = f - r * a.C;
            if (r < rows) {
                float s = a.scores[((int64_t)b * a.R + r) * a.lds + c];
                if (s > a.score_thr) {
                    v = true;
                    if (a.factors) s = s * a.factors[(int64_t)b * a.R + r];
                    key[k] = sort_key(fkey(s), f);
                    const float* p = box_of(a, b, r, c);
                    mk = max(mk, box_max_key(p[0], p[1], p[2], p[3]));
                    const u32 slot = atomicAdd(a.ccnt + (int64_t)b * a.ccnt_ld + c, 1u);
                    if ((int)slot < a.R) a.seg[((int64_t)b * a.C + c) * a.R + slot] = key[k];
                }
            }
        }
        const u64 bal = __ballot(v);
        before[k] = (u32)__popcll(bal & ((1ull << lane) - 1ull));
        valid |= v ? 1u << k : 0u;
        if (lane == 0) s_cnt[k * (kThreads / 64) + wv] = (u32)__popcll(bal);
    }
    __syncthreads();
    // one counter step per workgroup: the flat list's slots of (item, wave) in turn
    if (tid == 0) {
        u32 total = 0u;
        for (int i = 0; i < kFilterItems * (kThreads / 64); ++i) {
            const u32 n = s_cnt[i];
            s_cnt[i] = total;
            total += n;
        }
        s_base = total ? atomicAdd(hdr + kHdrM, total) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kFilterItems; ++k) {
        const u32 slot = s_base + s_cnt[k * (kThreads / 64) + wv] + before[k];
        if (((valid >> k) & 1u) && slot < (u32)kFlatCap && slot < (u32)a.n) a.list[(int64_t)b * a.n + slot] = key[k];
    }
    mk = wave_max_u(mk);
    if (lane == 0 && mk != 0u) atomicMax(hdr + kHdrMax, mk);
}

__global__ void __launch_bounds__(kThreads) mc_flat_rank_kernel(McArgs a) {
    __shared__ u64 s_tile[kRankTile];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int M = (int)a.hdr[b * kHdrWords + kHdrM];
    if (!all_pairs(M, a.split) || blockIdx.x * kThreads >= M) return;
    const u64* keys = a.list + (int64_t)b * a.n;
    const int i = blockIdx.x * kThreads + tid;
    const u64 my = i < M ? keys[i] : 0ull;
    const int rank = count_greater_tiled<kThreads>(keys, M, my, s_tile);
    if (i < M) a.ranked[(int64_t)b * kFlatCap + rank] = my;
}

// The greedy walk over the m ranked keys rk[0 .. m) (LDS or global) of image b on the shifted boxes, by a workgroup of T threads
// holding P boxes each (m <= T P).  FLAT: the kept keys go to sel[b] in rank order and their number to the header; else they are
// appended to the image's kept list.
template <int T, int P, bool FLAT>
__device__ __forceinline__ void walk(const McArgs& a, int b, const u64* rk, int m) {
    __shared__ f32x4 s_box[2][64];
    __shared__ u64 s_key[2][64];
    __shared__ u64 s_kept;
    __shared__ int s_total;
    const int tid = threadIdx.x;
    u32* hdr = a.hdr + b * kHdrWords;
    const float shift = fkey_inv(hdr[kHdrMax]) + 1.0f;
    const float off = a.offset, thr = a.thr;
    f32x4 box[P];
    u32 alive = 0u;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int j = k * T + tid;
        box[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (j < m) {
            const int f = key_index(rk[j]);
            const int r = f / a.C, c = f - r * a.C;
            const float* p = box_of(a, b, r, c);
            // batched_nms: offsets = idxs.to(boxes) * (boxes.max() + 1); boxes_for_nms = boxes + offsets[:, None]
            const float o = (float)c * shift;
            box[k] = f32x4{p[0] + o, p[1] + o, p[2] + o, p[3] + o};
            alive |= 1u << k;
        }
    }
    int total = 0;
    const int nrb = (m + 63) >> 6;
    for (int r = 0; r < nrb; ++r) {
        const int j0 = r * 64, slot = j0 / T, t0 = j0 - slot * T, buf = r & 1;
        if (tid >= t0 && tid < t0 + 64) {
            f32x4 v = box[0];
#pragma unroll
            for (int k = 1; k < P; ++k)
                if (k == slot) v = box[k];
            const int j = j0 + tid - t0;                                        // = slot * T + tid
            s_box[buf][tid - t0] = v;
            s_key[buf][tid - t0] = ((alive >> slot) & 1u) ? rk[j] : 0ull;       // 0: suppressed, or behind the end of the list
        }
        __syncthreads();
        if (tid < 64) {
            const int rows = min(64, m - j0);
            const f32x4 me = s_box[buf][tid];
            const float sa = nms_area(me, off);
            const u64 mykey = s_key[buf][tid];
            u64 word = 0ull;
            for (int c = 0; c < rows; ++c) {
                const f32x4 q = s_box[buf][c];
                const bool hit = nms_suppresses(me, sa, q, nms_area(q, off), off, thr) && c > tid;
                word |= hit ? (1ull << c) : 0ull;
            }
            const u64 kept = resolve_block64(word, ~__ballot(mykey != 0ull), a.cap - total);
            const int nk = __popcll(kept);
            u32 base = (u32)total;
            if (!FLAT && nk > 0) {
                if (tid == 0) base = atomicAdd(hdr + kHdrKept, (u32)nk);
                base = (u32)__builtin_amdgcn_readfirstlane((int)base);
            }
            if ((kept >> tid) & 1ull) {
                const u32 pos = base + (u32)__popcll(kept & ((1ull << tid) - 1ull));
                if (FLAT) a.sel[(int64_t)b * a.cap + pos] = mykey;
                else if (pos < (u32)a.n) a.list[(int64_t)b * a.n + pos] = mykey;
            }
            if (tid == 0) { s_kept = kept; s_total = total + nk; }
        }
        __syncthreads();
        const u64 kept = s_kept;
        total = s_total;
        if (total >= a.cap) break;                          // the rest of the walk cannot add a box
        if (alive) {
            for (u64 kk = kept; kk; kk &= kk - 1ull) {
                const int c = __ffsll((long long)kk) - 1;
                const f32x4 q = s_box[buf][c];
                const float sq = nms_area(q, off);
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    if (k * T + tid >= j0 + 64 && ((alive >> k) & 1u) && nms_suppresses_quick(q, sq, box[k], off, thr))
                        alive &= ~(1u << k);
                }
            }
        }
    }
    if (FLAT && tid == 0) hdr[kHdrSel] = (u32)total;
}

__global__ void __launch_bounds__(kFlatThreads) mc_flat_walk_kernel(McArgs a) {
    const int b = blockIdx.x;
    const int M = (int)a.hdr[b * kHdrWords + kHdrM];
    if (!all_pairs(M, a.split)) return;
    walk<kFlatThreads, kFlatPer, true>(a, b, a.ranked + (int64_t)b * kFlatCap, min(M, kFlatCap));
}

__global__ void __launch_bounds__(kClassThreads) mc_class_walk_kernel(McArgs a) {
    __shared__ u64 s_in[IIF_MULTICLASS_NMS_MAX_ROWS];
    __shared__ u64 s_rk[IIF_MULTICLASS_NMS_MAX_ROWS];
    const int tid = threadIdx.x, c = blockIdx.x, b = blockIdx.y;
    const int M = (int)a.hdr[b * kHdrWords + kHdrM];
    if (M == 0 || all_pairs(M, a.split)) return;
    const int m = min((int)a.ccnt[(int64_t)b * a.ccnt_ld + c], a.R);
    if (m == 0) return;
    const u64* seg = a.seg + ((int64_t)b * a.C + c) * a.R;
    u64 my[kClassPer];
#pragma unroll
    for (int k = 0; k < kClassPer; ++k) {
        const int j = k * kClassThreads + tid;
        my[k] = j < m ? seg[j] : 0ull;
        if (j < m) s_in[j] = my[k];
    }
    __syncthreads();
    int rank[kClassPer];
    count_greater_lds(s_in, m, my, rank);
#pragma unroll
    for (int k = 0; k < kClassPer; ++k)
        if (k * kClassThreads + tid < m) s_rk[rank[k]] = my[k];
    __syncthreads();
    walk<kClassThreads, kClassPer, false>(a, b, s_rk, m);
}

// select_pass_core's policy for image b: the cap largest of the K kept keys, the keys themselves as numbers; with at most cap
// kept keys everything is taken and the histogram passes return at once.
struct McSelect {
    struct Item { u64 number; };
    const McArgs& a; int seg, n, k; bool all;
    u32* hist; SelState* state; u32* hdr; const u64* keys;
    __device__ __forceinline__ McSelect(const McArgs& a_, int b, u32* hdr_, int K)
        : a(a_), seg(b), n(K), k(a_.cap), all(K <= a_.cap), hist(a_.hist), state(a_.state), hdr(hdr_), keys(a_.list + (int64_t)b * a_.n) {}
    __device__ __forceinline__ Item load(int i) const { return Item{keys[i]}; }
    __device__ __forceinline__ void take(int, const Item& it) const {
        const u32 slot = atomicAdd(hdr + kHdrSlot, 1u);
        if ((int)slot < k) a.sel[(int64_t)seg * k + slot] = it.number;
    }
    __device__ __forceinline__ void finish() const {}
};

__global__ void __launch_bounds__(kSelThreads) mc_select_kernel(McArgs a, int p) {
    const int b = blockIdx.y;
    u32* hdr = a.hdr + b * kHdrWords;
    const int M = (int)hdr[kHdrM];
    if (M == 0 || all_pairs(M, a.split)) return;
    const int K = min((int)hdr[kHdrKept], a.n);
    McSelect s(a, b, hdr, K);
    if (K == 0 || (s.all && p != kPasses)) return;
    select_pass_core(s, p);
}

__global__ void __launch_bounds__(kFinishThreads) mc_finish_kernel(McArgs a) {
    __shared__ u64 s_key[IIF_MULTICLASS_NMS_MAX_CAP];
    const int tid = threadIdx.x, b = blockIdx.x;
    const u32* hdr = a.hdr + b * kHdrWords;
    const int M = (int)hdr[kHdrM];
    int n = all_pairs(M, a.split) ? (int)hdr[kHdrSel] : min((int)hdr[kHdrKept], a.n);
    n = M == 0 ? 0 : min(n, a.cap);
    const u64* sel = a.sel + (int64_t)b * a.cap;
    for (int i = tid; i < n; i += kFinishThreads) s_key[i] = sel[i];
    __syncthreads();
    for (int i = tid; i < n; i += kFinishThreads) {
        const u64 my[1] = {s_key[i]};
        int rank[1];
        count_greater_lds(s_key, n, my, rank);
        const int f = key_index(my[0]);
        const int r = f / a.C, c = f - r * a.C;
        const float* p = box_of(a, b, r, c);
        const int64_t o = (int64_t)b * a.cap + rank[0];
        float* d = a.dets + o * 5;
        d[0] = p[0]; d[1] = p[1]; d[2] = p[2]; d[3] = p[3];
        d[4] = ranked_score(a, b, r, c);
        a.labels[o] = c;
        a.inds[o] = f;
    }
    for (int i = n + tid; i < a.cap; i += kFinishThreads) {
        const int64_t o = (int64_t)b * a.cap + i;
        zero_det_row(a.dets + o * 5);
        a.labels[o] = -1;
        a.inds[o] = -1;
    }
    if (tid == 0) {
        a.counts[b] = n;
        if (a.ncand) a.ncand[b] = M;
    }
}

}  // namespace

extern "C" int iif_multiclass_nms(const float* boxes, int64_t ld_boxes, int boxes_per_class, const float* scores, int64_t ld_scores,
                                  const float* score_factors, const int64_t* row_counts, int B, int64_t R, int64_t C,
                                  float score_thr, float iou_threshold, int offset, int64_t split_thr, int64_t cap, float* dets,
                                  int64_t* labels, int64_t* inds, int64_t* counts, int64_t* num_candidates, void* d_workspace,
                                  int64_t workspace_bytes, void* stream) {
    if (B < 1 || B > kMaxImages || R < 0 || R > IIF_MULTICLASS_NMS_MAX_ROWS || C < 1 || C > IIF_MULTICLASS_NMS_MAX_CLASSES) return IIF_EINVAL;
    const int64_t n = R * C;
    if (n >= (int64_t)1 << 24 || cap < 1 || cap > IIF_MULTICLASS_NMS_MAX_CAP || (offset != 0 && offset != 1)) return IIF_EINVAL;
    if (ld_scores < C + 1 || ld_boxes < (boxes_per_class ? 4 * C : 4)) return IIF_EINVAL;
    if (score_thr != score_thr || iou_threshold != iou_threshold) return IIF_EINVAL;
    if (split_thr > kFlatCap && n > kFlatCap) return IIF_EINVAL;          // the all-pairs regime holds at most kFlatCap candidates
    if (!scores || !dets || !labels || !inds || !counts || (R > 0 && !boxes)) return IIF_EINVAL;
    if (!aligned_to(boxes, 4) || !aligned_to(scores, 4) || !aligned_to(score_factors, 4) || !aligned_to(row_counts, 8) ||
        !aligned_to(dets, 4) || !aligned_to(labels, 8) || !aligned_to(inds, 8) || !aligned_to(counts, 8) || !aligned_to(num_candidates, 8))
        return IIF_EINVAL;
    if (!d_workspace || !aligned_to(d_workspace, 16) || workspace_bytes < IIF_MULTICLASS_NMS_WORKSPACE_BYTES(B, R, C, cap)) return IIF_EINVAL;
    McArgs a{};
    a.B = B; a.R = (int)R; a.C = (int)C; a.cap = (int)cap; a.n = (int)n;
    a.split = (int)(split_thr < 0 ? 0 : (split_thr > n + 1 ? n + 1 : split_thr));
    a.boxes = boxes; a.ldb = ld_boxes; a.per_class = boxes_per_class != 0;
    a.scores = scores; a.lds = ld_scores; a.factors = score_factors; a.row_counts = row_counts;
    a.score_thr = score_thr; a.thr = iou_threshold; a.offset = (float)offset;
    a.dets = dets; a.labels = labels; a.inds = inds; a.counts = counts; a.ncand = num_candidates;
    char* p = static_cast<char*>(d_workspace);
    a.hdr = reinterpret_cast<u32*>(p);
    a.state = reinterpret_cast<SelState*>(p + kStateOffset);
    p += kHeaderBytes;
    a.hist = reinterpret_cast<u32*>(p); p += B * kHistBytes;
    a.ccnt = reinterpret_cast<u32*>(p); a.ccnt_ld = (int)((C + 3) / 4 * 4); p += (int64_t)B * a.ccnt_ld * 4;
    const int64_t cleared = p - static_cast<char*>(d_workspace);
    a.ranked = reinterpret_cast<u64*>(p); p += (int64_t)B * kFlatCap * 8;
    a.seg = reinterpret_cast<u64*>(p); p += (int64_t)B * n * 8;
    a.list = reinterpret_cast<u64*>(p); p += (int64_t)B * n * 8;
    a.sel = reinterpret_cast<u64*>(p);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(d_workspace, 0, (size_t)cleared, st) != hipSuccess) return IIF_ELAUNCH;
    const unsigned fb = (unsigned)(n > 0 ? cdiv64(n, kThreads * kFilterItems) : 1);
    hipLaunchKernelGGL(mc_filter_kernel, dim3(fb, (unsigned)B), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    const unsigned rb = (unsigned)cdiv64(n < kFlatCap ? (n > 0 ? n : 1) : kFlatCap, kThreads);
    hipLaunchKernelGGL(mc_flat_rank_kernel, dim3(rb, (unsigned)B), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(mc_flat_walk_kernel, dim3((unsigned)B), dim3(kFlatThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(mc_class_walk_kernel, dim3((unsigned)C, (unsigned)B), dim3(kClassThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    for (int ps = 0; ps <= kPasses; ++ps) {
        hipLaunchKernelGGL(mc_select_kernel, dim3(kSelBlocks, (unsigned)B), dim3(kSelThreads), 0, st, a, ps);
        IIF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(mc_finish_kernel, dim3((unsigned)B), dim3(kFinishThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}
