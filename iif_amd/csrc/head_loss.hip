// The classification half of BBoxHead.loss (roi_heads/bbox_heads/bbox_head.py:266-283) without its host read: the softmax
// cross entropy of iif_head.hip with avg_factor = max(#{label_weights > 0}, 1) counted ON THE DEVICE, and the top-1 accuracy of
// the rows that count, out of the same launch.
//
// One 64-lane wave owns one row; the row (C <= 2048) lives in registers, a lane holding groups of 4 consecutive columns
// (16 bytes of fp32, 8 of bf16) at (j * 64 + lane) * 4.  A group is one vector access when the row pitch and the base allow it
// and the group is whole, else up to four guarded element accesses: C need not be a multiple of 4 and any pitch >= C works.
// The softmax runs in base 2 on v_exp_f32 as iif_head.hip's does, with the exponent formed from z - max and the target's own
// term kept out of the sum (see the row loop).  The kernels are latency / HBM-bound: no MFMA.
//
// A row of weight 0 (a padding row of roi_stage_targets_padded) is NOT READ: its gradient row is zeros and it takes no part in
// the loss, the count or the accuracy, whatever its scores or its label hold (the reference multiplies it by 0, which turns a
// non-finite padding row into NaN).  A row with a negative weight enters the loss but not the count, as in the reference.
//
// avg is known only when the last row is done, so the gradient is stored WITHOUT loss_weight / avg and iif_head_loss_bwd applies
// upstream * loss_weight / avg from the device scalars in its one launch (normed_mask_predictor.hip's device-scalar pattern).
//
// Reduction: loss_reduce.h's ticketed_sums carries three sums - the float loss sum and the INTEGER count of valid rows and of
// hits - to thread 0 of the last block, where head_loss_finish combines them into loss, acc and avg: a fixed order of
// additions for a given N, integers exact, no float atomics, the same bits every call.  Only the ticket word has to be zero on
// entry, and it is zero again on exit.
//
// iif_head_loss_cums_fwd (FasaIIFLoss with open accumulators, losses/fasa_iif_loss.py:145-160) is the ROWS instance of the same
// row loop - it also stores the row losses, counts the rows with w != 0 and returns their mean - followed by
// class_accumulate_rows_kernel, a wave per class that adds the stored rows of its class in ascending row order.  The instances
// of iif_head_loss_fwd are the ROWS = false ones: the same code as before the template parameter.
//
// iif_head_bce_loss_fwd (CrossEntropyLoss(use_sigmoid=True)) is the same frame around the sigmoid element of head_math.h that
// bce_head.hip uses: head_bce_kernel, below head_loss_kernel.  Both end in head_loss_finish, the reduction described above.
#include "common.h"
#include "head_math.h"
#include "loss_reduce.h"
#include "vec16.h"

namespace {

constexpr int kMaxBlocks = (IIF_HEAD_LOSS_WORKSPACE_BYTES / 4 - 4) / 3;       // partial triples behind the 4-word header
static_assert(IIF_HEAD_LOSS_WORKSPACE_BYTES == 4 * (4 + 3 * kMaxBlocks), "a 4-word header and whole (sum, valid, hits) triples");
static_assert(IIF_HEAD_LOSS_WORKSPACE_BYTES <= IIF_CE_WORKSPACE_BYTES, "the per-stream CE workspace serves this head too");

constexpr int kThreads = 256;            // the one block size of head_loss_kernel and head_bce_kernel: four waves, a row each
template <typename T> constexpr int kVecBytes = 4 * (int)sizeof(T);      // a group of 4 columns

struct HeadLossArgs {
    const void* x; int64_t ldx;
    const float* tab;                  // nullable: ones
    const int64_t* labels;
    const float* roww; const float* clsw;   // nullable: ones
    int64_t ignore; float loss_weight;
    int N, C;
    void* dx; int64_t lddx;            // nullable: loss only
    int32_t* status;
    float* loss_out; float* acc_out; float* avg_out;
    int32_t* ws;                       // [0] ticket, [1..3] unused, then (float sum, int valid, int hits) per block
    int vec_in, vec_out;               // whole groups of x / dx are one vector access
    float* rows_out;                   // ROWS instances only: the row losses [N]
};

// One group of 4 columns at c0 (a multiple of 4): a vector access if the row allows it.  Only the LAST group of a lane
// (j == NCH - 1) can be ragged or missing - NCH = ceil(C / 256) - so only that one (RAGGED) tests its columns: columns that do
// not exist read as -inf (they never win the max, add 0 to the sum and never outrank a target) and are never written.
template <typename T, bool RAGGED>
__device__ __forceinline__ void load_group(const T* row, int c0, int C, bool vec, float (&v)[4]) {
    if (vec && (!RAGGED || c0 + 4 <= C)) { VT<T>::load4(row + c0, v); return; }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (!RAGGED || c0 + e < C) ? VT<T>::load1(row + c0 + e) : -INFINITY;
}
template <typename T, bool RAGGED>
__device__ __forceinline__ void store_group(T* row, int c0, int C, bool vec, const float (&v)[4]) {
    if (vec && (!RAGGED || c0 + 4 <= C)) { VT<T>::store4(row + c0, v); return; }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (!RAGGED || c0 + e < C) VT<T>::store1(row + c0 + e, v[e]);
}

// The gradient row of a row that is not read
template <typename T, int NCH>
__device__ __forceinline__ void store_zero_row(T* dxr, int lane, int C, bool vec) {
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NCH - 1; ++j) store_group<T, false>(dxr, (j * 64 + lane) * 4, C, vec, zero);
    store_group<T, true>(dxr, ((NCH - 1) * 64 + lane) * 4, C, vec, zero);
}

// The end of both kernels, called by every thread with its wave's sums (wave-uniform): the grid's (sum, valid, hits) reach thread
// 0 of the last block (loss_reduce.h), which writes loss, acc and avg and puts the ticket word ws[0] back to zero.
// ROWS: loss_weight is already in the row losses that were summed.
template <bool ROWS>
__device__ __forceinline__ void head_loss_finish(const HeadLossArgs& a, float wave_loss, int wave_v, int wave_h) {
    float sum[1] = {wave_loss};
    int n[2] = {wave_v, wave_h};
    if (!ticketed_sums<1, 2, kThreads>(a.ws, a.ws + 4, sum, n)) return;
    const int valid = n[0], hits = n[1];
    const float avg = (float)(valid > 1 ? valid : 1);
    *a.loss_out = ROWS ? sum[0] / avg : a.loss_weight * (sum[0] / avg);
    // accuracy.py:49: correct.float().sum() * (100.0 / rows), the factor a Python double rounded to float32
    *a.acc_out = valid > 0 ? (float)hits * (float)(100.0 / (double)avg) : 0.f;
    *a.avg_out = avg;
    __hip_atomic_store(a.ws, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// NCH: groups per lane = ceil(C / 256).  Blocks of 4 waves; a wave walks rows wave, wave + n_waves, ...
// (launch bound: no occupancy asked for - 8 groups are 32 row values per lane, and the compiler's own allocation keeps every
// instance free of scratch; a tighter bound would only constrain it)
// ROWS (iif_head_loss_cums_fwd: FasaIIFLoss with open accumulators, reduction 'none' followed by .mean()): the row losses
// loss_weight * w_i * nll_i are stored (0 for a row that is not read), the rows that count are those with w != 0 - in the
// accuracy and in the divisor alike - and the loss is the sum of the stored rows over max(#{w != 0}, 1).
template <typename T, int NCH, bool ROWS>
__global__ void __launch_bounds__(256) head_loss_kernel(HeadLossArgs a) {
    // aligned(32), more than any other array of the block asks for, puts the table FIRST in LDS, where the row loop's reads of it
    // need no base: behind the reduction's arrays <float, 2, *> takes 82 VGPRs for 74 and loses a wave per SIMD
    __shared__ __attribute__((aligned(32))) float tab_s[NCH * 256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nwaves = gridDim.x * 4;
    const int C = a.C;
    for (int i = threadIdx.x; i < NCH * 256; i += 256) tab_s[i] = (a.tab != nullptr && i < C) ? a.tab[i] : 1.0f;
    __syncthreads();
    float wave_loss = 0.f;
    int wave_v = 0, wave_h = 0;                    // wave-uniform
    for (int row = blockIdx.x * 4 + wv; row < a.N; row += nwaves) {
        asm volatile("" ::: "memory");            // keep the table reads in LDS: hoisted into registers they cost the occupancy
        const float w = a.roww ? a.roww[row] : 1.0f;
        T* dxr = a.dx ? static_cast<T*>(a.dx) + (int64_t)row * a.lddx : nullptr;
        bool live = w != 0.f;                      // (a NaN weight is live, and poisons the loss as it does in the reference)
        int l = 0;
        if (live) {
            const int64_t l64 = a.labels[row];
            const bool in_range = l64 >= 0 && l64 < C;
            if (l64 != a.ignore && !in_range && a.status && lane == 0) atomicExch(a.status, 1);
            live = in_range && l64 != a.ignore;
            l = live ? (int)l64 : 0;
        }
        const bool counts = ROWS ? w != 0.f : w > 0.f;
        wave_v += counts;
        if (!live) {                               // wave-uniform: nothing of the row is read
            if (ROWS && lane == 0) a.rows_out[row] = 0.f;
            if (dxr) store_zero_row<T, NCH>(dxr, lane, C, a.vec_out);
            continue;
        }
        const T* xr = static_cast<const T*>(a.x) + (int64_t)row * a.ldx;
        float z[NCH][4];
#pragma unroll
        for (int j = 0; j < NCH - 1; ++j) load_group<T, false>(xr, (j * 64 + lane) * 4, C, a.vec_in, z[j]);
        load_group<T, true>(xr, ((NCH - 1) * 64 + lane) * 4, C, a.vec_in, z[NCH - 1]);
        const float xt = VT<T>::load1(xr + l);
        // top-1 on the RAW scores, iif_topk_hits' tie rule: columns that outrank the target, an equal score at a lower index included
        int cnt = 0;
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c0 = (j * 64 + lane) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cnt += (z[j][e] > xt) || (z[j][e] == xt && c0 + e < l);
                z[j][e] *= tab_s[c0 + e];
                m = fmaxf(m, z[j][e]);
            }
        }
        cnt = wave_sum_i(cnt);
        wave_h += counts && cnt == 0;
        m = wave_max(m);
        // 2^((z - m) log2 e) with the difference formed first, so that the row maximum contributes exactly 1 (iif_head.hip's single
        // fma z log2 e - round(m log2 e) scales the whole row by 2^residual: harmless for its lse = m + ..., not here).
        // The target's own term e_l stays OUT of the sum: with so = sum_{c != l} e_c,
        //   nll = log(so + e_l) - log(e_l) = log1p(so / e_l)      and      softmax_l - 1 = -so / (so + e_l),
        // neither of which cancels when the row is a confident hit (softmax_l -> 1: log(sum) and softmax_l - 1 would be right only
        // to ulp(1), far more than such a row's whole nll and gradient).
        float so = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c0 = (j * 64 + lane) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) z[j][e] = fast_exp2((z[j][e] - m) * kLog2e);
            const unsigned d = (unsigned)(l - c0);
            if (d < 4u) so += ((d == 0u ? 0.f : z[j][0]) + (d == 1u ? 0.f : z[j][1])) + ((d == 2u ? 0.f : z[j][2]) + (d == 3u ? 0.f : z[j][3]));
            else so += (z[j][0] + z[j][1]) + (z[j][2] + z[j][3]);
        }
        so = wave_sum(so);
        const float dl = xt * tab_s[l] - m;                       // <= 0, the same product the row's own element is
        const float el = fast_exp2(dl * kLog2e);
        const float sum = so + el, inv_s = 1.0f / sum;
        // (el underflows only for a target ~87 below the maximum: there log(sum) - dl has nothing to cancel)
        const float nll = el > 1e-30f ? log1pf(so / el) : kLn2 * fast_log2(sum) - dl;
        const float cw = a.clsw ? a.clsw[l] : 1.0f;
        if (ROWS) {
            const float r = a.loss_weight * (w * (cw * nll));
            if (lane == 0) a.rows_out[row] = r;
            wave_loss += r;
        } else {
            wave_loss += w * (cw * nll);
        }
        if (dxr == nullptr) continue;
        const float coef = w * cw, gs = coef * inv_s, gl = -(so * gs);
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c0 = (j * 64 + lane) * 4;
            float p[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = (c0 + e == l ? gl : z[j][e] * gs) * tab_s[c0 + e];
            if (j < NCH - 1) store_group<T, false>(dxr, c0, C, a.vec_out, p);
            else store_group<T, true>(dxr, c0, C, a.vec_out, p);
        }
    }
    head_loss_finish<ROWS>(a, wave_loss, wave_v, wave_h);
}

// The sigmoid head: mmdet's binary_cross_entropy with one class index per row (cross_entropy_loss.py:53-111, the element of
// bce_head.hip) in the frame of head_loss_kernel - a wave per row, the weight read first, the row in registers, the three sums.
// A label >= C that is valid is a background row (every column a negative), a label < 0 or equal to ignore_index turns the
// row's weight into 0 but the row still counts in V when label_weights > 0, as in the reference; a hit needs a label in [0, C).
template <typename T, int NCH>
__global__ void __launch_bounds__(256) head_bce_kernel(HeadLossArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nwaves = gridDim.x * 4;
    const int C = a.C;
    float wave_loss = 0.f;
    int wave_v = 0, wave_h = 0;                    // wave-uniform
    for (int row = blockIdx.x * 4 + wv; row < a.N; row += nwaves) {
        const float w = a.roww ? a.roww[row] : 1.0f;
        T* dxr = a.dx ? static_cast<T*>(a.dx) + (int64_t)row * a.lddx : nullptr;
        if (w == 0.f) {                            // wave-uniform: nothing of the row is read, its label included
            if (dxr) store_zero_row<T, NCH>(dxr, lane, C, a.vec_out);
            continue;
        }
        const int64_t l64 = a.labels[row];
        const bool valid = l64 >= 0 && l64 != a.ignore;
        const bool in_range = l64 >= 0 && l64 < C;
        const float wi = valid ? w : 0.0f;
        const int t = (valid && in_range) ? (int)l64 : -1;
        const T* xr = static_cast<const T*>(a.x) + (int64_t)row * a.ldx;
        float z[NCH][4];
#pragma unroll
        for (int j = 0; j < NCH - 1; ++j) load_group<T, false>(xr, (j * 64 + lane) * 4, C, a.vec_in, z[j]);
        load_group<T, true>(xr, ((NCH - 1) * 64 + lane) * 4, C, a.vec_in, z[NCH - 1]);
        const int lh = in_range ? (int)l64 : 0;
        const float xt = VT<T>::load1(xr + lh);
        int cnt = 0;
        float lsum = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c0 = (j * 64 + lane) * 4;
            float d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // top-1 on the raw scores, iif_topk_hits' tie rule (columns that do not exist hold -inf and never outrank)
                cnt += (z[j][e] > xt) || (z[j][e] == xt && c0 + e < lh);
                float l;
                bce_label_elem(z[j][e], c0 + e, t, wi, a.clsw, l, d[e]);
                if (j < NCH - 1 || c0 + e < C) lsum += l;
            }
            if (dxr == nullptr) continue;
            if (j < NCH - 1) store_group<T, false>(dxr, c0, C, a.vec_out, d);
            else store_group<T, true>(dxr, c0, C, a.vec_out, d);
        }
        cnt = wave_sum_i(cnt);
        wave_loss += wave_sum(lsum);
        wave_v += w > 0.f;
        wave_h += w > 0.f && in_range && cnt == 0;
    }
    head_loss_finish<false>(a, wave_loss, wave_v, wave_h);
}

// out = u * (upstream * loss_weight / avg), the three factors read on the device
template <typename T>
__global__ void __launch_bounds__(256) head_loss_scale_kernel(const T* u, int64_t n, const float* upstream, const float* avg, float loss_weight,
                                                              T* out, int vec) {
    const float f = (*upstream * loss_weight) / *avg;
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (vec) {
        const int64_t n4 = n / 4;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
            float v[4];
            VT<T>::load4(u + 4 * i, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= f;
            VT<T>::store4(out + 4 * i, v);
        }
        for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) VT<T>::store1(out + i, VT<T>::load1(u + i) * f);
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) VT<T>::store1(out + i, VT<T>::load1(u + i) * f);
    }
}

// wave = class c: cum_labels[c] += #{i: labels[i] == c, w_i != 0}, cum_losses[c] += the sum of rows[i] over those i in ASCENDING
// row order (FasaIIFLoss.forward, losses/fasa_iif_loss.py:154-160).  The wave looks at 64 labels at a time; the rows of a ballot
// are added one by one, lowest first, by every lane alike (plain adds, no atomics: the same bits every call).
__global__ void __launch_bounds__(256) class_accumulate_rows_kernel(const float* rows, const int64_t* labels, const float* roww, int n,
                                                                    int C, float* cum_losses, float* cum_labels) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;                                      // wave-uniform
    float s = 0.f;
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool hit = i < n && labels[i] == (int64_t)c && (roww == nullptr || roww[i] != 0.f);
        unsigned long long m = __ballot(hit);
        cnt += __popcll(m);
        while (m) {
            s += rows[i0 + __builtin_ctzll(m)];
            m &= m - 1;
        }
    }
    if (cnt && lane == 0) { cum_losses[c] += s; cum_labels[c] += (float)cnt; }
}

// The two kernel families of the forward entries
template <bool ROWS> struct SoftmaxKernels { template <typename T, int NCH> static constexpr auto kernel = head_loss_kernel<T, NCH, ROWS>; };
struct SigmoidKernels { template <typename T, int NCH> static constexpr auto kernel = head_bce_kernel<T, NCH>; };

template <typename F, typename T>
int launch_rows(HeadLossArgs a, hipStream_t st) {
    a.vec_in = a.N > 0 && a.ldx % 4 == 0 && aligned(a.x, kVecBytes<T>);
    a.vec_out = a.dx != nullptr && a.lddx % 4 == 0 && aligned(a.dx, kVecBytes<T>);
    int blocks = (a.N + 3) / 4;
    if (blocks < 1) blocks = 1;                   // N == 0: one block writes loss 0, acc 0, avg 1
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    const dim3 grid(blocks), block(kThreads);
    switch ((a.C + 255) / 256) {                  // 1 .. 8: the entries refuse C > 2048
    case 1: hipLaunchKernelGGL((F::template kernel<T, 1>), grid, block, 0, st, a); break;      // COCO: 81, sigmoid 80
    case 2: hipLaunchKernelGGL((F::template kernel<T, 2>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((F::template kernel<T, 3>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((F::template kernel<T, 4>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL((F::template kernel<T, 5>), grid, block, 0, st, a); break;      // LVIS: 1204, Seesaw-sized 1205, sigmoid 1203
    case 6: hipLaunchKernelGGL((F::template kernel<T, 6>), grid, block, 0, st, a); break;
    case 7: hipLaunchKernelGGL((F::template kernel<T, 7>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((F::template kernel<T, 8>), grid, block, 0, st, a); break;
    }
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}
template <typename F>
int launch_rows(int dtype, const HeadLossArgs& a, void* stream) {
    return dtype == IIF_F32 ? launch_rows<F, float>(a, as_stream(stream)) : launch_rows<F, unsigned short>(a, as_stream(stream));
}

// What the three forward entries ask of their arguments, IIF_EINVAL before IIF_EUNSUPPORTED.  outs: every result pointer of the
// entry is there; ins: so is everything that N > 0 rows are read from or written to.
int check_fwd(int dtype, int N, int C, int min_C, const void* scores, int64_t ld_scores, const void* dscores, int64_t ld_dscores, bool outs,
              bool ins, const void* d_workspace) {
    if (N < 0 || N > IIF_HEAD_LOSS_MAX_ROWS || C < min_C) return IIF_EINVAL;
    if (dtype != IIF_F32 && dtype != IIF_BF16) return IIF_EINVAL;
    if (!outs || !d_workspace || !aligned(d_workspace, 4)) return IIF_EINVAL;
    if (N > 0 && !ins) return IIF_EINVAL;
    if (N > 0 && (ld_scores < C || (dscores && ld_dscores < C))) return IIF_EINVAL;
    if (!aligned(scores, dtype == IIF_F32 ? 4 : 2) || !aligned(dscores, dtype == IIF_F32 ? 4 : 2)) return IIF_EINVAL;
    if (C > IIF_HEAD_LOSS_MAX_CLASSES) return IIF_EUNSUPPORTED;
    return IIF_OK;
}

}  // namespace

extern "C" {

int iif_head_bce_loss_fwd(const void* scores, int dtype, int64_t ld_scores, const int64_t* labels, const float* label_weights,
                          const float* class_weight, int64_t ignore_index, float loss_weight, int N, int C, void* dscores,
                          int64_t ld_dscores, float* loss_out, float* acc_out, float* avg_out, void* d_workspace, void* stream) {
    const int rc = check_fwd(dtype, N, C, 1, scores, ld_scores, dscores, ld_dscores, loss_out && acc_out && avg_out, scores && labels,
                             d_workspace);
    if (rc != IIF_OK) return rc;
    HeadLossArgs a{scores, ld_scores, nullptr, labels, label_weights, class_weight, ignore_index, loss_weight, N, C,
                   N > 0 ? dscores : nullptr, ld_dscores, nullptr, loss_out, acc_out, avg_out, static_cast<int32_t*>(d_workspace), 0, 0,
                   nullptr};
    return launch_rows<SigmoidKernels>(dtype, a, stream);
}

int iif_head_loss_fwd(const void* scores, int dtype, int64_t ld_scores, const float* table, const int64_t* labels,
                      const float* label_weights, const float* class_weight, int64_t ignore_index, float loss_weight, int N, int C,
                      void* dscores, int64_t ld_dscores, float* loss_out, float* acc_out, float* avg_out, int32_t* d_status,
                      void* d_workspace, void* stream) {
    const int rc = check_fwd(dtype, N, C, 2, scores, ld_scores, dscores, ld_dscores, loss_out && acc_out && avg_out, scores && labels,
                             d_workspace);
    if (rc != IIF_OK) return rc;
    HeadLossArgs a{scores, ld_scores, table, labels, label_weights, class_weight, ignore_index, loss_weight, N, C,
                   N > 0 ? dscores : nullptr, ld_dscores, d_status, loss_out, acc_out, avg_out, static_cast<int32_t*>(d_workspace), 0, 0,
                   nullptr};
    return launch_rows<SoftmaxKernels<false>>(dtype, a, stream);
}

int iif_head_loss_cums_fwd(const void* scores, int dtype, int64_t ld_scores, const float* table, const int64_t* labels,
                           const float* label_weights, const float* class_weight, int64_t ignore_index, float loss_weight, int N, int C,
                           void* dscores, int64_t ld_dscores, float* rows_out, float* cum_losses, float* cum_labels, float* loss_out,
                           float* acc_out, float* avg_out, int32_t* d_status, void* d_workspace, void* stream) {
    int rc = check_fwd(dtype, N, C, 2, scores, ld_scores, dscores, ld_dscores, loss_out && acc_out && avg_out && cum_losses && cum_labels,
                       scores && labels && rows_out, d_workspace);
    if (rc != IIF_OK) return rc;
    HeadLossArgs a{scores, ld_scores, table, labels, label_weights, class_weight, ignore_index, loss_weight, N, C,
                   N > 0 ? dscores : nullptr, ld_dscores, d_status, loss_out, acc_out, avg_out, static_cast<int32_t*>(d_workspace), 0, 0,
                   rows_out};
    rc = launch_rows<SoftmaxKernels<true>>(dtype, a, stream);
    if (rc != IIF_OK || N == 0) return rc;
    hipLaunchKernelGGL(class_accumulate_rows_kernel, dim3((C + 3) / 4), dim3(256), 0, as_stream(stream), rows_out, labels, label_weights,
                       N, C, cum_losses, cum_labels);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_head_loss_bwd(const void* dscores, int dtype, int64_t n, const float* d_upstream, const float* d_avg, float loss_weight,
                      void* out, void* stream) {
    if (n < 0 || !d_upstream || !d_avg) return IIF_EINVAL;
    if (dtype != IIF_F32 && dtype != IIF_BF16) return IIF_EINVAL;
    if (n == 0) return IIF_OK;
    if (!dscores || !out) return IIF_EINVAL;
    const int es = dtype == IIF_F32 ? 4 : 2;
    if (!aligned(dscores, es) || !aligned(out, es)) return IIF_EINVAL;
    const int vec = aligned(dscores, 4 * es) && aligned(out, 4 * es);
    const int64_t want = cdiv64(vec ? cdiv64(n, 4) : n, 256);
    const int blocks = (int)(want < 2048 ? want : 2048);
    if (dtype == IIF_F32)
        hipLaunchKernelGGL(head_loss_scale_kernel<float>, dim3(blocks), dim3(256), 0, as_stream(stream), (const float*)dscores, n,
                           d_upstream, d_avg, loss_weight, (float*)out, vec);
    else
        hipLaunchKernelGGL(head_loss_scale_kernel<unsigned short>, dim3(blocks), dim3(256), 0, as_stream(stream),
                           (const unsigned short*)dscores, n, d_upstream, d_avg, loss_weight, (unsigned short*)out, vec);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // extern "C"
