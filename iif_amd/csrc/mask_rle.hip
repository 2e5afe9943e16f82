// COCO run-length encoding on the device for gfx950 (MI355X): the counts of pycocotools' rleEncode for pasted masks straight from
// the [h, w] logits tile and the box (iif_paste_rle_*: the boolean image of iif_paste_masks never exists), and for bitmaps that are
// already on the device (iif_mask_rle_*).
//
// The mask is read in column-major order, pixel j = x * H + y.  A TRANSITION sits at j when M[j] != M[j - 1], with M[-1] := 0; the
// counts are the differences of successive transition positions, opened by 0 and closed by H * W, so a mask with T transitions
// has T + 1 counts.  Three passes, each a pure function of its inputs (no atomics: the same bytes from call to call):
//
//   count   an item is (mask, column, segment of kSegRows rows); lanes run along x, each lane walks down its column and counts its
//           transitions.  A pasted mask is the constant `fill` outside the conservative rectangle of mask_paste.h, so only the
//           columns [xlo, min(xhi + 1, W - 1)] and rows [ylo, min(yhi + 1, H - 1)] are walked, plus column 0 and row 0 where
//           they are not among them (M[-1] = 0 against fill = 1 at threshold 0, and a run that crosses from the bottom of one
//           column into the top of the next); the pixel itself is paste_pixel, the definition iif_paste_masks uses.  The tile
//           goes through the sigmoid into LDS once per block.  A bitmap walks every column and row, lanes along x: coalesced.
//   scan    one block per mask turns its item counts into exclusive offsets in place, in column-major item order, and writes
//           totals[n] = T + 1; a last block turns the totals into the masks' offsets in the flat run buffer.
//   fill    the count pass again, now writing each transition's POSITION at its offset (and H * W behind the last one); one
//           differencing launch then forms  runs[k] = pos[k] - pos[k - 1].
//
// The host reads totals [N] between scan and fill to allocate the exact run buffer: the test end finishes on the host anyway.
#include "common.h"
#include "mask_paste.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / IIF_WAVE;
constexpr int kSegRows = 128;                 // rows of one item

// The columns and rows of one mask that can hold a transition: [c0, c0 + nc) and [r0, r0 + nr), preceded by column 0 / row 0
// where c0 / r0 > 0 (then counted in ncols / nrows).  Items are (column index, segment) with the segment fastest.
struct RleGeom {
    int c0, ncols, r0, nrows, nseg;
    __device__ __forceinline__ int col(int c) const { return (c0 > 0 && c == 0) ? 0 : c0 + c - (c0 > 0); }
    __device__ __forceinline__ int row(int r) const { return (r0 > 0 && r == 0) ? 0 : r0 + r - (r0 > 0); }
};

__device__ __forceinline__ RleGeom rle_geom(int xlo, int xhi, int ylo, int yhi, int H, int W) {
    RleGeom g;
    const int x1 = min(xhi + 1, W - 1), y1 = min(yhi + 1, H - 1);
    g.c0 = xlo; g.r0 = ylo;
    g.ncols = max(0, x1 - xlo + 1) + (xlo > 0);
    g.nrows = max(0, y1 - ylo + 1) + (ylo > 0);
    g.nseg = (g.nrows + kSegRows - 1) / kSegRows;
    return g;
}

struct RleArgs {
    int H, W, seg_groups;                     // seg_groups: blocks along the rows of a mask (kWaves segments each)
    int64_t ws_stride;                        // items of one mask in the workspace: W * ceil(H / kSegRows) at most
    int32_t* ws;
    int32_t* totals;
    int64_t* offsets;                         // [N + 1] (in the workspace)
    int64_t N;
    uint32_t* pos;
    uint32_t* runs;
    int64_t cap;                              // entries of pos and runs
};

// ---- pixel sources: geometry(n) is uniform over the block and touches no LDS; load() fills LDS (the caller synchronises);
// pixel(x, y) is M[y, x]
struct PasteSrc {
    const void* pred; int dtype, activated;
    const int64_t* labels;
    const float* boxes; int64_t ldb;
    int C, h, w, img_h, img_w;
    float thr;
    PasteBox b;
    int64_t c;

    __device__ __forceinline__ RleGeom geometry(int64_t n) {
        const bool valid = paste_box(boxes + n * ldb, labels, n, C, h, w, img_h, img_w, thr, &b, &c);
        b.any = valid && b.xhi >= b.xlo && b.yhi >= b.ylo;
        // no pixel is evaluated: the whole mask is `fill`, and (0, 0) is the one place where a transition can sit
        if (!b.any) return rle_geom(1, -1, 1, -1, img_h, img_w);
        return rle_geom(b.xlo, b.xhi, b.ylo, b.yhi, img_h, img_w);
    }
    __device__ __forceinline__ void load(int64_t n, float* tile, int tid) {
        if (b.any) paste_load_tile(pred, dtype, activated, (n * C + c) * (h * w), h * w, tile, tid, kThreads);
    }
    __device__ __forceinline__ uint8_t pixel(const float* tile, int x, int y) const { return paste_pixel(b, tile, y, x); }
};

struct BitmapSrc {
    const uint8_t* p; int64_t ld_row, ld_mask;
    int H, W;
    const uint8_t* m;

    __device__ __forceinline__ RleGeom geometry(int64_t n) {
        m = p + n * ld_mask;
        return rle_geom(0, W - 1, 0, H - 1, H, W);
    }
    __device__ __forceinline__ void load(int64_t, float*, int) {}
    __device__ __forceinline__ uint8_t pixel(const float*, int x, int y) const { return m[(int64_t)y * ld_row + x] != 0; }
};

template <class Src> struct TileOf { static constexpr int kFloats = 1; };
template <> struct TileOf<PasteSrc> { static constexpr int kFloats = kMaxPred * kMaxPred; };

// FILL false: ws[item] = transitions of the item.  FILL true: ws holds the exclusive offsets; positions go to pos.
template <class Src, bool FILL>
__global__ void __launch_bounds__(kThreads) rle_walk_kernel(Src src, RleArgs a) {
    __shared__ float tile[TileOf<Src>::kFloats];
    const int tid = threadIdx.x;
    const int lane = tid & (IIF_WAVE - 1), wave = tid >> 6;
    const int64_t n = blockIdx.y;
    const int chunk = (int)blockIdx.x / a.seg_groups, sg = (int)blockIdx.x - chunk * a.seg_groups;
    const RleGeom g = src.geometry(n);
    if (chunk * IIF_WAVE >= g.ncols || sg * kWaves >= g.nseg) return;           // uniform over the block
    src.load(n, tile, tid);
    __syncthreads();
    const int c = chunk * IIF_WAVE + lane, s = sg * kWaves + wave;
    if (c >= g.ncols || s >= g.nseg) return;
    const int x = g.col(c);
    const int ra = s * kSegRows, rb = min(g.nrows, ra + kSegRows);
    const int64_t item = n * a.ws_stride + (int64_t)c * g.nseg + s;
    uint32_t* pos = nullptr;
    int64_t room = 0;                         // entries from this mask's offset to the end of the buffer the caller allocated
    int k = 0;
    if (FILL) { pos = a.pos + a.offsets[n]; room = a.cap - a.offsets[n]; k = a.ws[item]; }
    int yprev = -2;
    uint8_t pv = 0;
    for (int r = ra; r < rb; ++r) {
        const int y = g.row(r);
        uint8_t before = pv;
        if (y != yprev + 1)                                                      // the item's first row, or the row after row 0
            before = y > 0 ? src.pixel(tile, x, y - 1) : (x > 0 ? src.pixel(tile, x - 1, a.H - 1) : (uint8_t)0);
        const uint8_t cur = src.pixel(tile, x, y);
        if (cur != before) {
            if (FILL && k >= 0 && k < room) pos[k] = (uint32_t)x * (uint32_t)a.H + (uint32_t)y;
            ++k;
        }
        pv = cur; yprev = y;
    }
    if (!FILL) a.ws[item] = k;
    else if (c == g.ncols - 1 && s == g.nseg - 1 && k >= 0 && k < room) pos[k] = (uint32_t)a.H * (uint32_t)a.W;      // closes the last run
}

template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < IIF_WAVE; o <<= 1) {
        const T u = __shfl_up(v, o, IIF_WAVE);
        if (lane >= o) v += u;
    }
    return v;
}

// Inclusive scan of one value per thread over the block; *total: the block's sum.  `sh`: kWaves values.
template <class T>
__device__ __forceinline__ T block_inclusive_scan(T v, T* sh, int tid, T* total) {
    const int lane = tid & (IIF_WAVE - 1), wave = tid >> 6;
    v = wave_inclusive_scan(v, lane);
    __syncthreads();                                                             // sh of the previous round has been read
    if (lane == IIF_WAVE - 1) sh[wave] = v;
    __syncthreads();
    T add = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        if (i < wave) add += sh[i];
        sum += sh[i];
    }
    *total = sum;
    return v + add;
}

// block n < N: the items of mask n -> exclusive offsets in place, totals[n] = transitions + 1
template <class Src>
__global__ void __launch_bounds__(kThreads) rle_scan_kernel(Src src, RleArgs a) {
    __shared__ int sh[kWaves];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x;
    const RleGeom g = src.geometry(n);
    const int items = g.ncols * g.nseg;
    int32_t* ws = a.ws + n * a.ws_stride;
    int carry = 0;
    for (int i0 = 0; i0 < items; i0 += kThreads) {
        const int i = i0 + tid;
        const int v = i < items ? ws[i] : 0;
        int total;
        const int inc = block_inclusive_scan(v, sh, tid, &total);
        if (i < items) ws[i] = carry + inc - v;
        carry += total;
    }
    if (tid == 0) a.totals[n] = carry + 1;
}

// offsets[n] = totals[0] + ... + totals[n - 1] for n in [0, N]
__global__ void __launch_bounds__(kThreads) rle_offsets_kernel(RleArgs a) {
    __shared__ int64_t sh[kWaves];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int64_t i0 = 0; i0 < a.N; i0 += kThreads) {
        const int64_t i = i0 + tid;
        const int64_t v = i < a.N ? a.totals[i] : 0;
        int64_t total;
        const int64_t inc = block_inclusive_scan(v, sh, tid, &total);
        if (i < a.N) a.offsets[i] = carry + inc - v;
        carry += total;
    }
    if (tid == 0) a.offsets[a.N] = carry;
}

// runs[k] = pos[k] - pos[k - 1] within each mask (pos[-1] = 0); one thread per run, its mask found by bisection of the offsets
__global__ void __launch_bounds__(kThreads) rle_diff_kernel(RleArgs a, int64_t total) {
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= total) return;
    int64_t lo = 0, hi = a.N;                                                    // offsets[lo] <= k < offsets[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.offsets[mid] <= k) lo = mid; else hi = mid;
    }
    const uint32_t p = a.pos[k];
    a.runs[k] = k == a.offsets[lo] ? p : p - a.pos[k - 1];
}

int64_t seg_count(int H) { return cdiv64(H, kSegRows); }

// the item arrays of N masks, then offsets [N + 1] as int64 on an 8-byte boundary
int64_t items_bytes(int64_t N, int H, int W) { return (N * (int64_t)W * seg_count(H) * 4 + 7) / 8 * 8; }

int prepare(RleArgs* a, int64_t N, int H, int W, void* workspace, int64_t workspace_bytes, int32_t* totals) {
    if (!workspace || !aligned_to(workspace, 8) || !totals || !aligned_to(totals, 4)) return IIF_EINVAL;
    if (workspace_bytes < items_bytes(N, H, W) + (N + 1) * 8) return IIF_EINVAL;
    a->H = H; a->W = W; a->N = N;
    a->seg_groups = (int)cdiv64(seg_count(H), kWaves);
    a->ws_stride = (int64_t)W * seg_count(H);
    a->ws = static_cast<int32_t*>(workspace);
    a->offsets = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + items_bytes(N, H, W));
    a->totals = totals;
    return IIF_OK;
}

dim3 walk_grid(const RleArgs& a) { return dim3((unsigned)(cdiv64(a.W, IIF_WAVE) * a.seg_groups), (unsigned)a.N); }

template <class Src>
int run_count(const Src& src, const RleArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((rle_walk_kernel<Src, false>), walk_grid(a), dim3(kThreads), 0, st, src, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL((rle_scan_kernel<Src>), dim3((unsigned)a.N), dim3(kThreads), 0, st, src, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(rle_offsets_kernel, dim3(1), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

template <class Src>
int run_fill(const Src& src, RleArgs a, int64_t total, uint32_t* positions, uint32_t* runs, hipStream_t st) {
    if (total < a.N || !positions || !aligned_to(positions, 4) || !runs || !aligned_to(runs, 4)) return IIF_EINVAL;
    a.pos = positions; a.runs = runs; a.cap = total;
    hipLaunchKernelGGL((rle_walk_kernel<Src, true>), walk_grid(a), dim3(kThreads), 0, st, src, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(rle_diff_kernel, dim3((unsigned)cdiv64(total, kThreads)), dim3(kThreads), 0, st, a, total);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

// iif_paste_masks' checks, in its order; IIF_OK with *empty set: nothing to enqueue
int paste_src(PasteSrc* s, const void* mask_pred, int dtype, int activated, const int64_t* labels, const float* boxes, int64_t ld_boxes,
              int64_t N, int C, int h, int w, int img_h, int img_w, float threshold, bool* empty) {
    *empty = false;
    if (N < 0 || N > 65535 || C <= 0 || h <= 0 || w <= 0 || img_h <= 0 || img_w <= 0 || ld_boxes < 4) return IIF_EINVAL;
    if (dtype != IIF_F32 && dtype != IIF_BF16) return IIF_EINVAL;
    if (!(threshold >= 0.0f)) return IIF_EINVAL;                        // negative (the uint8 visualisation branch) or NaN
    if (h > kMaxPred || w > kMaxPred || (int64_t)img_h * img_w > INT32_MAX) return IIF_EUNSUPPORTED;
    if (N == 0) { *empty = true; return IIF_OK; }
    if (!mask_pred || !aligned_to(mask_pred, dtype == IIF_BF16 ? 2 : 4) || !boxes || !aligned_to(boxes, 4)) return IIF_EINVAL;
    if (labels && !aligned_to(labels, 8)) return IIF_EINVAL;
    *s = PasteSrc{};
    s->pred = mask_pred; s->dtype = dtype; s->activated = activated != 0; s->labels = labels; s->boxes = boxes; s->ldb = ld_boxes;
    s->C = C; s->h = h; s->w = w; s->img_h = img_h; s->img_w = img_w; s->thr = threshold;
    return IIF_OK;
}

int bitmap_src(BitmapSrc* s, const uint8_t* masks, int64_t ld_row, int64_t ld_mask, int64_t N, int H, int W, bool* empty) {
    *empty = false;
    if (N < 0 || N > 65535 || H <= 0 || W <= 0) return IIF_EINVAL;
    if (ld_row < W || ld_mask < (int64_t)(H - 1) * ld_row + W) return IIF_EINVAL;
    if ((int64_t)H * W > INT32_MAX) return IIF_EUNSUPPORTED;
    if (N == 0) { *empty = true; return IIF_OK; }
    if (!masks) return IIF_EINVAL;
    *s = BitmapSrc{};
    s->p = masks; s->ld_row = ld_row; s->ld_mask = ld_mask; s->H = H; s->W = W;
    return IIF_OK;
}

}  // namespace

extern "C" {

int64_t iif_rle_workspace_bytes(int64_t N, int H, int W) {
    if (N < 0 || H <= 0 || W <= 0) return 0;
    return items_bytes(N, H, W) + (N + 1) * 8;
}

int iif_paste_rle_count(const void* mask_pred, int dtype, int activated, const int64_t* labels, const float* boxes, int64_t ld_boxes,
                        int64_t N, int C, int h, int w, int img_h, int img_w, float threshold, void* workspace,
                        int64_t workspace_bytes, int32_t* totals, void* stream) {
    PasteSrc src; RleArgs a{}; bool empty;
    int rc = paste_src(&src, mask_pred, dtype, activated, labels, boxes, ld_boxes, N, C, h, w, img_h, img_w, threshold, &empty);
    if (rc != IIF_OK || empty) return rc;
    if ((rc = prepare(&a, N, img_h, img_w, workspace, workspace_bytes, totals)) != IIF_OK) return rc;
    return run_count(src, a, as_stream(stream));
}

int iif_paste_rle_fill(const void* mask_pred, int dtype, int activated, const int64_t* labels, const float* boxes, int64_t ld_boxes,
                       int64_t N, int C, int h, int w, int img_h, int img_w, float threshold, void* workspace,
                       int64_t workspace_bytes, const int32_t* totals, int64_t total, uint32_t* positions, uint32_t* runs,
                       void* stream) {
    PasteSrc src; RleArgs a{}; bool empty;
    int rc = paste_src(&src, mask_pred, dtype, activated, labels, boxes, ld_boxes, N, C, h, w, img_h, img_w, threshold, &empty);
    if (rc != IIF_OK || empty) return rc;
    if ((rc = prepare(&a, N, img_h, img_w, workspace, workspace_bytes, const_cast<int32_t*>(totals))) != IIF_OK) return rc;
    return run_fill(src, a, total, positions, runs, as_stream(stream));
}

int iif_mask_rle_count(const uint8_t* masks, int64_t ld_row, int64_t ld_mask, int64_t N, int H, int W, void* workspace,
                       int64_t workspace_bytes, int32_t* totals, void* stream) {
    BitmapSrc src; RleArgs a{}; bool empty;
    int rc = bitmap_src(&src, masks, ld_row, ld_mask, N, H, W, &empty);
    if (rc != IIF_OK || empty) return rc;
    if ((rc = prepare(&a, N, H, W, workspace, workspace_bytes, totals)) != IIF_OK) return rc;
    return run_count(src, a, as_stream(stream));
}

int iif_mask_rle_fill(const uint8_t* masks, int64_t ld_row, int64_t ld_mask, int64_t N, int H, int W, void* workspace,
                      int64_t workspace_bytes, const int32_t* totals, int64_t total, uint32_t* positions, uint32_t* runs,
                      void* stream) {
    BitmapSrc src; RleArgs a{}; bool empty;
    int rc = bitmap_src(&src, masks, ld_row, ld_mask, N, H, W, &empty);
    if (rc != IIF_OK || empty) return rc;
    if ((rc = prepare(&a, N, H, W, workspace, workspace_bytes, const_cast<int32_t*>(totals))) != IIF_OK) return rc;
    return run_fill(src, a, total, positions, runs, as_stream(stream));
}

}  // extern "C"
