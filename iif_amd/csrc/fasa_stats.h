// The arithmetic of the FASA feature bank, shared by fasa.hip (the rows already compacted by the caller) and fasa_head.hip
// (padded rows, positives selected on the device): whatever finds a class's rows, ONE function turns them into the bank's
// mean and variance, so the two kernels agree bit for bit by construction (the library is built with -ffp-contract=off:
// nothing here is fused behind the source's back).
//
// Reference: fa_update_push, roi_heads/bbox_heads/fasa_bbox_head.py:131-148; fa_generate, :160-162.
#pragma once
#include "common.h"

// One (class, feature) pair.  for_each_row(visit) calls visit(i) for every row i of the class in ASCENDING order, `total`
// (>= 1) of them; it is called twice, so a row's value is read twice.  Plain adds for the sum, sum / total, the centred sum
// of squares with fmaf(t, t, ss), var(unbiased=False) * n / (n - 1) for n > 1 (:133-137), then first sight -> copy, afterwards
// the moving average (:139-147).  col = emb + d, m / v = the pair's slots in feature_mean / feature_std.
template <typename ForEachRow>
__device__ __forceinline__ void fasa_class_feature(const float* col, int64_t lde, int total, bool seen, float decay, float* m, float* v,
                                                   ForEachRow for_each_row) {
    float sum = 0.f;
    for_each_row([&](int i) { sum += col[(int64_t)i * lde]; });
    const float mean = sum / (float)total;
    float ss = 0.f;
    for_each_row([&](int i) { const float t = col[(int64_t)i * lde] - mean; ss = fmaf(t, t, ss); });
    const float var = total > 1 ? (ss / (float)total) * ((float)total / (float)(total - 1)) : ss / (float)total;
    if (seen) {
        *m = decay * mean + (1.f - decay) * *m;
        *v = decay * var + (1.f - decay) * *v;
    } else {
        *m = mean;
        *v = var;
    }
}

// One element of a virtual embedding (:160-162)
__device__ __forceinline__ float fasa_virtual_sample(float mean, float var, float normal) { return mean + sqrtf(var) * normal; }

// Is class c drawn this step (:152, :158)?
__device__ __forceinline__ bool fasa_class_drawn(const float* rnd, const float* prob, const float* fused, int c) {
    return rnd[c] < prob[c] && fused[c] > 0.f;
}
