// The per-class segment sum of per-RoI gradient rows, shared by the class-selected mask predictor (mask_predictor.hip) and the
// fused mask head tail (mask_tail.hip): scratch [n][cin + 1] -> dweight [C][cin], dbias [C].
#pragma once
#include "common.h"

namespace {

// One block per class: the labels pass through LDS 256 at a time and leave the ascending list of the class's RoIs (ballot and
// prefix count: no sort), then every thread adds the scratch rows of that list for its columns, eight loads in flight, the
// additions in list order.  Writes every row of dweight and every element of dbias.
__global__ void __launch_bounds__(256) mask_predict_dw_classes_kernel(const float* __restrict__ scratch,
                                                                      const int64_t* __restrict__ labels, int n, int cin,
                                                                      float* __restrict__ dweight, float* __restrict__ dbias) {
    constexpr int kPiece = 2048;
    __shared__ int list[kPiece];
    __shared__ int wcnt[4];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ld = cin + 1;
    for (int col0 = 0; col0 < ld; col0 += 256) {
        const int col = col0 + tid;
        float acc = 0.f;
        for (int n0 = 0; n0 < n; n0 += kPiece) {
            const int m = min(kPiece, n - n0);
            int cnt = 0;                                 // block-uniform
            for (int i0 = 0; i0 < m; i0 += 256) {
                const int i = i0 + tid;
                const bool hit = i < m && labels[n0 + i] == k;
                const unsigned long long b = __ballot(hit);
                __syncthreads();                         // the previous round's wcnt (and, first round, the previous list) is read
                if (lane == 0) wcnt[wv] = __popcll(b);
                __syncthreads();
                int off = cnt;
                for (int w = 0; w < wv; ++w) off += wcnt[w];
                if (hit) list[off + __popcll(b & ((1ull << lane) - 1ull))] = n0 + i;
                cnt += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            }
            __syncthreads();
            if (col < ld) {
                const float* sc = scratch + col;
                int j = 0;
                for (; j + 8 <= cnt; j += 8) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = sc[(int64_t)list[j + u] * ld];
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc += v[u];
                }
                for (; j < cnt; ++j) acc += sc[(int64_t)list[j] * ld];
            }
        }
        if (col < cin) { if (dweight) dweight[(int64_t)k * cin + col] = acc; }
        else if (col == cin) { if (dbias) dbias[k] = acc; }
    }
}

}  // namespace
