// FasaBBoxHead.loss without a host read, gfx950: the feature bank fed from PADDED rows and virtual embeddings of a fixed shape.
//
// Reference (instance_segmentation/mmdet/models/roi_heads/bbox_heads/fasa_bbox_head.py):
//   :258-262  pos_embedding = embedding[pos_inds]; fa_update(pos_embedding, labels[pos_inds])   two boolean indexings = two host reads
//   :284-299  fa_generate(); len(aug_embedding); aug_avg_factor = ....item()                    a row count that depends on the draw
//
// iif_fasa_update_rows   grid (class, chunk of 256 features).  A block finds the rows of ITS class by an ordered scan of the
//   labels (a ballot per wave, the wave totals through LDS): the first kRowCap row indices go to LDS in ascending order, a class
//   with more rows finds the rest by walking the labels on from the last listed row.  Thread d then hands that row walk to
//   fasa_stats.h's fasa_class_feature, the function fasa.hip's kernel uses: the same adds in the same order, the same bits as
//   fa_update on the compacted rows.  Only rows whose label is the block's class are dereferenced - a padding row, a background
//   row or a negative label is never read - and each of them twice (two-pass variance).  Integer work: N label reads per block;
//   nothing is C x N over the embedding.  No atomics at all.  feature_used is bumped by a second, tiny launch (a class's blocks
//   all have to see the value from BEFORE this update; block (c, 0) leaves "class c was present" in `present`).
//
// iif_fasa_generate_padded   ONE launch, block k = output row k.  Every block scans `rnd < prob && used > 0` over the classes
//   itself (C ~ 1e3: five ballots) and so knows the class of rank k and the number drawn; rows at or beyond the count are zeros
//   with label C and weight 0.  The element is fasa_stats.h's fasa_virtual_sample, as in fasa.hip.
//
// Both are latency-bound index work followed by streaming reads: no MFMA, a few hundred bytes of LDS, 256-thread blocks.
#include "common.h"
#include "fasa_stats.h"

namespace {

constexpr int kRowCap = 1024;      // row indices of one class kept in LDS (N <= 65535: 16 bits each)

__global__ void __launch_bounds__(256) fasa_update_rows_kernel(const float* emb, const int64_t* labels, int n, int D, int64_t lde,
                                                               float decay, float* fmean, float* fvar, const float* fused,
                                                               int32_t* present) {
    __shared__ unsigned short list[kRowCap];
    __shared__ int wtot[4];
    const int c = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int total = 0;                                           // block-uniform
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool hit = i < n && labels[i] == (int64_t)c;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wtot[wv] = __popcll(m);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < 4; ++w) { woff += w < wv ? wtot[w] : 0; tot += wtot[w]; }
        const int pos = total + woff + __popcll(m & ((1ull << lane) - 1ull));
        if (hit && pos < kRowCap) list[pos] = (unsigned short)i;
        total += tot;
        __syncthreads();                                     // wtot is rewritten by the next chunk; list is complete after the last
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) present[c] = total > 0;
    if (total == 0) return;
    const int d = blockIdx.y * 256 + threadIdx.x;
    if (d >= D) return;
    const bool seen = fused[c] > 0.f;
    const int listed = total < kRowCap ? total : kRowCap;
    const int64_t o = (int64_t)c * D + d;
    fasa_class_feature(emb + d, lde, total, seen, decay, fmean + o, fvar + o, [&](auto visit) {
        for (int k = 0; k < listed; ++k) visit((int)list[k]);
        if (total > kRowCap)
            for (int i = (int)list[kRowCap - 1] + 1; i < n; ++i)
                if (labels[i] == (int64_t)c) visit(i);
    });
}

// thread c: first sight of a class that was present (fa_update_push :148)
__global__ void __launch_bounds__(256) fasa_mark_used_kernel(const int32_t* present, int C, float* fused) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C && present[c] && !(fused[c] > 0.f)) fused[c] += 1.f;
}

__global__ void __launch_bounds__(256) fasa_generate_padded_kernel(const float* rnd, const float* prob, const float* fused,
                                                                   const float* fmean, const float* fvar, const float* normal, int C,
                                                                   int D, int K, float aug_weight, float* out, int64_t* out_labels,
                                                                   float* out_weights, int32_t* count) {
    __shared__ int wtot[4];
    __shared__ int mine_s;
    const int k = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) mine_s = -1;
    int drawn = 0;                                           // block-uniform: classes drawn below c0
    for (int c0 = 0; c0 < C; c0 += 256) {
        const int c = c0 + threadIdx.x;
        const bool take = c < C && fasa_class_drawn(rnd, prob, fused, c);
        const unsigned long long m = __ballot(take);
        if (lane == 0) wtot[wv] = __popcll(m);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < 4; ++w) { woff += w < wv ? wtot[w] : 0; tot += wtot[w]; }
        if (take && drawn + woff + __popcll(m & ((1ull << lane) - 1ull)) == k) mine_s = c;      // at most one thread, once
        drawn += tot;
        __syncthreads();
    }
    const int c = mine_s;                                    // -1: fewer than k + 1 classes drawn
    if (k == 0 && threadIdx.x == 0) {
        count[0] = drawn < K ? drawn : K;
        count[1] = drawn < K ? 0 : drawn - K;                // classes dropped for want of capacity
    }
    for (int d = threadIdx.x; d < D; d += 256) {
        const int64_t o = (int64_t)c * D + d;
        out[(int64_t)k * D + d] = c >= 0 ? fasa_virtual_sample(fmean[o], fvar[o], normal[o]) : 0.f;
    }
    if (threadIdx.x == 0) {
        out_labels[k] = c >= 0 ? c : C;
        out_weights[k] = c >= 0 ? aug_weight : 0.f;
    }
}

}  // namespace

extern "C" {

int iif_fasa_update_rows(const float* embedding, const int64_t* labels, int n, int d, int64_t ld, int c, float decay,
                         float* feature_mean, float* feature_var, float* feature_used, int32_t* present, void* stream) {
    if (n < 0 || d <= 0 || c <= 0 || ld < d) return IIF_EINVAL;
    if (n > IIF_FASA_ROWS_MAX_ROWS || c > IIF_FASA_ROWS_MAX_CLASSES) return IIF_EUNSUPPORTED;
    if (n == 0) return IIF_OK;
    if (!embedding || !labels || !feature_mean || !feature_var || !feature_used || !present) return IIF_EINVAL;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(fasa_update_rows_kernel, dim3(c, (d + 255) / 256), dim3(256), 0, st, embedding, labels, n, d, ld, decay,
                       feature_mean, feature_var, feature_used, present);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(fasa_mark_used_kernel, dim3((c + 255) / 256), dim3(256), 0, st, present, c, feature_used);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_fasa_generate_padded(const float* rnd, const float* prob, const float* feature_used, const float* feature_mean,
                             const float* feature_var, const float* normal, int c, int d, int capacity, float aug_weight, float* out,
                             int64_t* out_labels, float* out_weights, int32_t* count, void* stream) {
    if (c <= 0 || d <= 0 || capacity < 1) return IIF_EINVAL;
    if (!rnd || !prob || !feature_used || !feature_mean || !feature_var || !normal || !out || !out_labels || !out_weights || !count)
        return IIF_EINVAL;
    hipLaunchKernelGGL(fasa_generate_padded_kernel, dim3(capacity), dim3(256), 0, as_stream(stream), rnd, prob, feature_used,
                       feature_mean, feature_var, normal, c, d, capacity, aug_weight, out, out_labels, out_weights, count);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // extern "C"
