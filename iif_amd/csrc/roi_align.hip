// SingleRoIExtractor for gfx950 (MI355X): the FPN level mapping, the optional roi rescaling and mmcv's RoIAlign (pool_mode 'avg')
// in one launch over all levels, forward and backward.
//
//   iif_roi_extract_forward    instance_segmentation/mmdet/models/roi_heads/roi_extractors/single_level_roi_extractor.py:37-115
//                              (map_roi_levels, the per-level nonzero / gather / RoIAlign / index_put) + base_roi_extractor.py:62-84
//                              (roi_rescale) + mmcv's roi_align forward.
//   iif_roi_extract_backward   one clear of the arena that holds every level's gradient + one launch of float atomic adds.
//
// Mapping.  A block is (roi, group of 64 channels, chunk of up to kChunkBins bins); the 64 lanes of a wave run over CHANNELS of
// the NHWC features, so every feature load and every atomic wave-instruction is 256 contiguous bytes - the one atomic shape
// that runs at the chip-wide rate.  The four waves share the chunk's bins.  The NCHW output tile (and the same tile of grad_out
// in backward) goes through LDS and is written (read) contiguously.
//
// Arithmetic.  Every coordinate is the reference's float32 expression in its order (the build passes -ffp-contract=off): level,
// rescaling, roi start / size / bin size, grid counts and each sample coordinate  y = start + ph * bin + (iy + .5f) * bin / grid;
// the drop rule (y < -1 || y > H), both clamps, the cell (int)y and the weights ly = y - y_low, hy = 1 - ly come from that y.
// The bin is then summed in SEPARABLE form: per axis the weight of pixel p is  W[p] = sum over kept samples of (hy if y_low == p)
// + (ly if y_high == p),  and  bin = sum_py sum_px Wy[py] Wx[px] f[py, px] / count  - a sample counts only when both axes keep it,
// which is the product.  A bin touches each distinct pixel once ((grid_h + 2)(grid_w + 2) at most when samples are at most one
// pixel apart) instead of 4 grid_h grid_w corner visits.  The per-axis weights are computed lane-parallel (lane j: pixel lo + j)
// and broadcast with v_readlane; a zero weight skips the pixel.  Only the summation order differs from mmcv's loop.
//
// Rows that produce zeros and no gradient: a batch index outside [0, N) (NaN included), a NaN scale with more than one level
// (negative area product; the reference leaves such a row at its new_zeros value), a non-finite coordinate, and a grid count
// above kMaxGrid on either axis (a roi side of more than 65536 bins' worth of feature pixels).
#include "common.h"
#include "roi_geom.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / IIF_WAVE;
constexpr int kMaxLevels = 8;
constexpr int kChunkBins = 224;               // bins per block: the LDS tile is kChunkBins x kTileLd floats (56.9 KiB at most)
constexpr int kTileLd = IIF_WAVE + 1;         // padded: the transposed read walks rows
constexpr int kMaxGrid = 65536;
constexpr int kMaxPooled = 1024;

struct Levels {
    float* p[kMaxLevels];                     // forward: features (read only); backward: gradients
    int H[kMaxLevels], W[kMaxLevels];
    float s[kMaxLevels];
};

struct RoiArgs {
    Levels lv;
    int L, N, C, PH, PW, sampling_ratio, aligned, out_cl;
    const float* rois; int64_t ld; int64_t K;
    float finest_scale, factor;
    float* out;                               // forward: output; backward: grad_out (read only)
    int32_t* lvl_out;
};

struct Geom {
    bool skip;
    int lvl, lvl_report, n, H, W, grid_h, grid_w;
    float start_h, start_w, bin_h, bin_w, count;
};

// Everything that depends on the roi alone.  Uniform over the block.
__host__ __device__ __forceinline__ Geom roi_geometry(const RoiArgs& a, int64_t k) {
    Geom g;
    const float* r = a.rois + k * a.ld;
    const float b = r[0];
    float x1 = r[1], y1 = r[2], x2 = r[3], y2 = r[4];
    g.skip = !(b >= 0.0f && b < (float)a.N) || !finite_f(x1) || !finite_f(y1) || !finite_f(x2) || !finite_f(y2);
    g.n = g.skip ? 0 : (int)b;
    g.lvl = 0;
    g.lvl_report = 0;
    if (a.L > 1) {                            // map_roi_levels, on the roi as given
        const float scale = sqrtf((x2 - x1) * (y2 - y1));
        const float t = floorf(log2f(scale / a.finest_scale + 1e-6f));
        if (t != t) {
            g.skip = true;
            g.lvl_report = -1;
        } else {
            const float hi = (float)(a.L - 1);
            g.lvl = (int)(t < 0.0f ? 0.0f : (t > hi ? hi : t));
            g.lvl_report = g.lvl;
        }
    }
    if (a.factor > 0.0f) {                    // roi_rescale
        const float cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f;
        const float w = x2 - x1, h = y2 - y1;
        const float nw = w * a.factor, nh = h * a.factor;
        x1 = cx - nw * 0.5f; x2 = cx + nw * 0.5f;
        y1 = cy - nh * 0.5f; y2 = cy + nh * 0.5f;
    }
    g.H = a.lv.H[g.lvl]; g.W = a.lv.W[g.lvl];
    const float s = a.lv.s[g.lvl];
    const float off = a.aligned ? 0.5f : 0.0f;
    g.start_w = x1 * s - off; g.start_h = y1 * s - off;
    const float end_w = x2 * s - off, end_h = y2 * s - off;
    float roi_w = end_w - g.start_w, roi_h = end_h - g.start_h;
    if (!a.aligned) {
        roi_w = fmaxf(roi_w, 1.0f);
        roi_h = fmaxf(roi_h, 1.0f);
    }
    g.bin_h = roi_h / (float)a.PH;
    g.bin_w = roi_w / (float)a.PW;
    const float gh = a.sampling_ratio > 0 ? (float)a.sampling_ratio : ceilf(roi_h / (float)a.PH);
    const float gw = a.sampling_ratio > 0 ? (float)a.sampling_ratio : ceilf(roi_w / (float)a.PW);
    if (!(gh <= (float)kMaxGrid && gw <= (float)kMaxGrid) || !finite_f(g.start_h) || !finite_f(g.start_w)) g.skip = true;
    g.grid_h = g.skip ? 0 : (int)gh;
    g.grid_w = g.skip ? 0 : (int)gw;
    const int64_t cnt = (int64_t)g.grid_h * g.grid_w;
    if (cnt > INT32_MAX) g.skip = true;
    g.count = (float)(cnt > 1 ? cnt : 1);
    return g;
}

__device__ __forceinline__ float lane_value(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// One bin of one roi for the wave's 64 channels.  BWD: adds gval * weight / count into the level's gradient; else returns the
// bin's value.  base: the image's pixel (0, 0) at the lane's channel; live: the lane has a channel.
template <bool BWD>
__device__ __forceinline__ float roi_bin(const Geom& g, int ph, int pw, float* base, int C, bool live, int lane, float gval) {
    float acc = 0.0f;
    int ylo, yhi, xlo, xhi;
    if (g.grid_h <= 0 || g.grid_w <= 0) return acc;
    if (!axis_range(g.start_h, g.bin_h, g.grid_h, ph, g.H, &ylo, &yhi)) return acc;
    if (!axis_range(g.start_w, g.bin_w, g.grid_w, pw, g.W, &xlo, &xhi)) return acc;
    for (int ry = ylo; ry <= yhi; ry += IIF_WAVE) {
        const float wyv = axis_weight(g.start_h, g.bin_h, g.grid_h, ph, g.H, ry + lane);
        const int ny = yhi - ry + 1 < IIF_WAVE ? yhi - ry + 1 : IIF_WAVE;
        for (int rx = xlo; rx <= xhi; rx += IIF_WAVE) {
            const float wxv = axis_weight(g.start_w, g.bin_w, g.grid_w, pw, g.W, rx + lane);
            const int nx = xhi - rx + 1 < IIF_WAVE ? xhi - rx + 1 : IIF_WAVE;
            for (int iy = 0; iy < ny; ++iy) {
                const float wy = lane_value(wyv, iy);
                if (wy == 0.0f) continue;
                float* row = base + ((int64_t)(ry + iy) * g.W + rx) * C;
                for (int ix = 0; ix < nx; ++ix) {
                    const float w = wy * lane_value(wxv, ix);
                    if (w == 0.0f || !live) continue;
                    if (BWD) atomicAdd(row + (int64_t)ix * C, gval * w / g.count);
                    else acc += w * row[(int64_t)ix * C];
                }
            }
        }
    }
    return BWD ? 0.0f : acc / g.count;
}

template <bool BWD>
__global__ void __launch_bounds__(kThreads) roi_extract_kernel(RoiArgs a) {
    extern __shared__ float tile[];           // [bins of the chunk][kTileLd]; unused with a channels-last output / grad_out
    const int64_t k = blockIdx.x;
    const int c0 = (int)blockIdx.y * IIF_WAVE;
    const int phw = a.PH * a.PW;
    const int b0 = (int)blockIdx.z * kChunkBins;
    const int nb = phw - b0 < kChunkBins ? phw - b0 : kChunkBins;
    const int nc = a.C - c0 < IIF_WAVE ? a.C - c0 : IIF_WAVE;
    const int lane = threadIdx.x & (IIF_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool live = lane < nc;
    const Geom g = roi_geometry(a, k);
    const int64_t nchw0 = (k * a.C + c0) * phw + b0;          // element (channel c0 + c, bin b0 + j): nchw0 + c * phw + j
    if (!BWD && a.lvl_out && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) a.lvl_out[k] = g.lvl_report;
    if (BWD) {
        if (g.skip) return;
        if (!a.out_cl) {
            for (int e = threadIdx.x; e < nc * nb; e += kThreads) {
                const int c = e / nb, j = e - c * nb;
                tile[j * kTileLd + c] = a.out[nchw0 + (int64_t)c * phw + j];
            }
            __syncthreads();
        }
    }
    float* base = g.skip ? nullptr : a.lv.p[g.lvl] + (int64_t)g.n * g.H * g.W * a.C + c0 + (live ? lane : 0);
    for (int j = wave; j < nb; j += kWaves) {
        const int b = b0 + j, ph = b / a.PW, pw = b - ph * a.PW;
        const int64_t cl = (k * phw + b) * a.C + c0 + lane;
        if (BWD) {
            const float gval = a.out_cl ? (live ? a.out[cl] : 0.0f) : tile[j * kTileLd + lane];
            roi_bin<true>(g, ph, pw, base, a.C, live, lane, gval);
        } else {
            const float v = g.skip ? 0.0f : roi_bin<false>(g, ph, pw, base, a.C, live, lane, 0.0f);
            if (a.out_cl) {
                if (live) a.out[cl] = v;
            } else {
                tile[j * kTileLd + lane] = v;
            }
        }
    }
    if (!BWD && !a.out_cl) {
        __syncthreads();
        for (int e = threadIdx.x; e < nc * nb; e += kThreads) {
            const int c = e / nb, j = e - c * nb;
            a.out[nchw0 + (int64_t)c * phw + j] = tile[j * kTileLd + c];
        }
    }
}

bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

// The checks both entries share; IIF_OK with *noop set for K == 0
int fill_args(RoiArgs* a, const iif_roi_level* levels, int num_levels, int N, int C, const float* rois, int64_t ld_rois, int64_t K,
              int pooled_h, int pooled_w, int sampling_ratio, int aligned, float finest_scale, float roi_scale_factor, bool* noop) {
    *noop = false;
    if (!levels || num_levels < 1 || num_levels > kMaxLevels || N <= 0 || C <= 0 || K < 0 || K > INT32_MAX || ld_rois < 5) return IIF_EINVAL;
    if (pooled_h <= 0 || pooled_w <= 0 || pooled_h > kMaxPooled || pooled_w > kMaxPooled || (int64_t)cdiv64(C, IIF_WAVE) > 65535) return IIF_EINVAL;
    if (num_levels > 1 && !(finest_scale > 0.0f)) return IIF_EINVAL;
    if (roi_scale_factor != roi_scale_factor) return IIF_EINVAL;
    for (int i = 0; i < num_levels; ++i) {
        const iif_roi_level& l = levels[i];
        if (l.H <= 0 || l.W <= 0 || !(l.spatial_scale > 0.0f) || l.spatial_scale > 3.0e38f) return IIF_EINVAL;
    }
    if (K == 0) {
        *noop = true;
        return IIF_OK;
    }
    if (!rois || !aligned4(rois)) return IIF_EINVAL;
    for (int i = 0; i < num_levels; ++i) {
        const iif_roi_level& l = levels[i];
        if (!l.ptr || !aligned4(l.ptr)) return IIF_EINVAL;
        a->lv.p[i] = static_cast<float*>(l.ptr); a->lv.H[i] = l.H; a->lv.W[i] = l.W; a->lv.s[i] = l.spatial_scale;
    }
    a->L = num_levels; a->N = N; a->C = C; a->PH = pooled_h; a->PW = pooled_w;
    a->sampling_ratio = sampling_ratio; a->aligned = aligned != 0;
    a->rois = rois; a->ld = ld_rois; a->K = K;
    a->finest_scale = finest_scale; a->factor = roi_scale_factor;
    return IIF_OK;
}

template <bool BWD>
int launch(const RoiArgs& a, hipStream_t st) {
    const int phw = a.PH * a.PW;
    const dim3 grid((unsigned)a.K, (unsigned)cdiv64(a.C, IIF_WAVE), (unsigned)cdiv64(phw, kChunkBins));
    const int nb = phw < kChunkBins ? phw : kChunkBins;
    const size_t lds = a.out_cl ? 0 : (size_t)nb * kTileLd * sizeof(float);
    hipLaunchKernelGGL(roi_extract_kernel<BWD>, grid, dim3(kThreads), lds, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // namespace

extern "C" {

int iif_roi_extract_forward(const iif_roi_level* levels, int num_levels, int N, int C, const float* rois, int64_t ld_rois,
                            int64_t K, int pooled_h, int pooled_w, int sampling_ratio, int aligned, float finest_scale,
                            float roi_scale_factor, float* out, int out_channels_last, int32_t* lvl_out, void* stream) {
    RoiArgs a{};
    bool noop;
    const int rc = fill_args(&a, levels, num_levels, N, C, rois, ld_rois, K, pooled_h, pooled_w, sampling_ratio, aligned,
                             finest_scale, roi_scale_factor, &noop);
    if (rc != IIF_OK || noop) return rc;
    if (!out || !aligned4(out) || !aligned4(lvl_out)) return IIF_EINVAL;
    a.out = out; a.out_cl = out_channels_last != 0; a.lvl_out = lvl_out;
    return launch<false>(a, as_stream(stream));
}

int iif_roi_extract_backward(const iif_roi_level* grad_levels, int num_levels, int N, int C, const float* rois, int64_t ld_rois,
                             int64_t K, int pooled_h, int pooled_w, int sampling_ratio, int aligned, float finest_scale,
                             float roi_scale_factor, const float* grad_out, int grad_channels_last, void* arena,
                             int64_t arena_bytes, void* stream) {
    RoiArgs a{};
    bool noop;
    const int rc = fill_args(&a, grad_levels, num_levels, N, C, rois, ld_rois, K, pooled_h, pooled_w, sampling_ratio, aligned,
                             finest_scale, roi_scale_factor, &noop);
    if (rc != IIF_OK || noop) return rc;
    if (!grad_out || !aligned4(grad_out) || !arena || arena_bytes <= 0) return IIF_EINVAL;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(arena), hi = lo + (uintptr_t)arena_bytes;
    for (int i = 0; i < num_levels; ++i) {    // every level's gradient lies in the arena that is cleared
        const uintptr_t p = reinterpret_cast<uintptr_t>(grad_levels[i].ptr);
        const uint64_t bytes = (uint64_t)N * grad_levels[i].H * grad_levels[i].W * C * sizeof(float);
        if (p < lo || p > hi || bytes > hi - p) return IIF_EINVAL;
    }
    a.out = const_cast<float*>(grad_out); a.out_cl = grad_channels_last != 0;
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(arena, 0, (size_t)arena_bytes, st) != hipSuccess) return IIF_ELAUNCH;
    return launch<true>(a, st);
}

}  // extern "C"
