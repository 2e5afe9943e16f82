// Fused Seesaw loss (Wang et al., CVPR 2021) for the LVIS bbox head on gfx950 (MI355X): the native path of mmdet's
// SeesawLoss plugin (instance_segmentation/mmdet/models/losses/seesaw_loss.py).
//
// cls_score is [N, C + 2] fp32: C class columns and two objectness columns.  A forward call is two launches:
//   1. seesaw_count_kernel   integer histogram of the labels (LDS atomics, then integer global atomics and a ticketed last
//                            block), added to cum_samples as ONE fp32 addition per class, plus the number of positive rows;
//   2. seesaw_loss_kernel    one 64-lane wave per row, the row in registers: both softmaxes, the seesaw terms in the log domain,
//                            the whole [N, C + 2] gradient, the per-row losses and both scalar losses (loss_reduce.h).
// Layout: the LVIS row is 1205 floats, so consecutive rows start on every 16-byte phase and no 16-byte vector path applies.
// Lane l of chunk j owns column j * 64 + l: each wave instruction is a dword access over 256 contiguous bytes, whatever the
// row's phase; only the last chunk is ragged (lanes beyond C hold -inf).  The kernels are latency / HBM bound: no GEMM, no MFMA.
// Arithmetic: base-2 hardware transcendentals (v_exp_f32 / v_log_f32, ~1 ulp), as in iif_head.hip.
// iif_seesaw_head_fwd (BBoxHead.loss without its host read) is the HEAD instance of the same two kernels: rows of weight 0 are
// not read, avg_factor is counted by the first launch, both accuracies and the division leave the second.
#include <math.h>

#include "common.h"
#include "head_math.h"
#include "loss_reduce.h"

namespace {

constexpr int kMaxCols = 2048;              // C + 2 <= 2048: the row stays in registers (<= 32 values per lane)
constexpr int kMaxLossBlocks = 1024;        // partial slots of the workspace
constexpr int kHeadThreads = 256;           // the one block size iif_seesaw_head_fwd launches the loss kernel with
constexpr int kCountBlock = 1024;           // threads of a count block
constexpr int kLabelsPerCountBlock = 16384;   // one block: 3.4 us at 1024 labels; four blocks with their atomics and ticket: 9.2 us at 8192
constexpr int kMaxCountBlocks = 64;
// workspace (int32 words): [0] loss ticket, [1] count ticket, [2] positive rows of the last call, [3] unused,
// [4, 4 + 2048) histogram (zero between calls), then 2 * kMaxLossBlocks floats of per-block partial sums
constexpr int kWsHist = 4;
constexpr int kWsPartial = kWsHist + kMaxCols;
static_assert(IIF_SEESAW_WORKSPACE_BYTES == 4 * (kWsPartial + 2 * kMaxLossBlocks), "header and kernel disagree on the workspace");
// workspace of iif_seesaw_head_fwd: the same four words and histogram, then [kWsHeadV] rows with w > 0 and [kWsHeadV + 1] positive
// rows with w > 0 of the last call, [kWsHeadV + 2 .. 3] their accumulators across count blocks (zero between calls), then per loss
// block (float class sum, float objectness sum, int objectness hits, int class hits)
constexpr int kWsHeadV = kWsHist + kMaxCols;
constexpr int kWsHeadPartial = kWsHeadV + 4;
static_assert(IIF_SEESAW_HEAD_WORKSPACE_BYTES == 4 * (kWsHeadPartial + 4 * kMaxLossBlocks), "header and kernel disagree on the workspace");

// ------------------------------------------------------------------------------------------------ count
// cum_samples[l] += (float)count(labels == l): the count is an integer, so the result does not depend on the order of
// anything and stays exact above 2^24 (three +1.0f onto 16777216.0f would be lost, one +3 gives 16777220).
//
// HEAD (iif_seesaw_head_fwd): a row of weight 0 is not counted and its label is not read - the weight, read first, gates the
// label's load, and such a row is handled as the rows past the end are.  The launch also counts V = #{w > 0} and the positive
// rows among them (0 <= label < C), into ws[kWsHeadV] and ws[kWsHeadV + 1].  The HEAD = false instance is the code that it was
// before the parameter.
template <bool HEAD>
__global__ void __launch_bounds__(kCountBlock) seesaw_count_kernel(const int64_t* labels, const float* roww, int N, int C, float* cum,
                                                                   int update, int32_t* ws, int32_t* status) {
    __shared__ int h[kMaxCols];
    __shared__ int last, npos;
    __shared__ int head_n[2];                      // HEAD: rows with w > 0, positive rows with w > 0
    const int nb = C + 1;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) h[i] = 0;
    if (threadIdx.x == 0) npos = 0;
    if (HEAD && threadIdx.x < 2) head_n[threadIdx.x] = 0;
    __syncthreads();
    int nv = 0, npw = 0;                           // HEAD: this thread's share of the two
    // the background is most of a sampled batch (mmdet: three rows in four): counted per lane and added once per wave, so the
    // LDS atomics do not queue on one address
    bool bad = false;
    int bg = 0;
    // eight labels per trip, their loads issued together: one dependent load per label made the latency of the label reads
    // the whole kernel (8.5 us for 8192 labels in one block)
    const int stride = gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < N; i0 += 8 * stride) {
        int64_t l[8];
        float w[8];
        if constexpr (HEAD) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int64_t i = i0 + (int64_t)k * stride;
                w[k] = i < N ? (roww ? roww[i] : 1.0f) : 0.0f;
                nv += w[k] > 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t i = i0 + (int64_t)k * stride;
            const bool there = HEAD ? w[k] != 0.f : i < N;
            l[k] = there ? labels[i] : (int64_t)C;         // past the end: a background label that is taken off again below
            if (!there) --bg;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (l[k] == C) ++bg;
            else if (l[k] >= 0 && l[k] < C) {
                atomicAdd(&h[(int)l[k]], 1);
                if (HEAD) npw += w[k] > 0.f;
            } else bad = true;
        }
    }
    bg = wave_sum_i(bg);
    if (bg != 0 && (threadIdx.x & 63) == 0) atomicAdd(&h[C], bg);
    if (bad && status) atomicExch(status, 1);
    if constexpr (HEAD) {
        nv = wave_sum_i(nv);
        npw = wave_sum_i(npw);
        if ((threadIdx.x & 63) == 0) {
            if (nv != 0) atomicAdd(&head_n[0], nv);
            if (npw != 0) atomicAdd(&head_n[1], npw);
        }
    }
    __syncthreads();
    if (gridDim.x > 1) {
        // integer global atomics (returning: complete when the value is back), then the ticket; the last block reads the
        // sums with agent-scope loads and leaves the histogram zero for the next call
        int32_t* gh = ws + kWsHist;
        int back = 0;
        for (int i = threadIdx.x; i < nb; i += blockDim.x)
            if (h[i] != 0) back += __hip_atomic_fetch_add(gh + i, h[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (HEAD && threadIdx.x < 2)               // the two row counts travel the same way, through ws[kWsHeadV + 2 .. 3]
            back += __hip_atomic_fetch_add(ws + kWsHeadV + 2 + threadIdx.x, head_n[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" : : "v"(back) : "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            const int t = __hip_atomic_fetch_add(ws + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = (t == (int)gridDim.x - 1);
        }
        __syncthreads();
        if (!last) return;
        for (int i = threadIdx.x; i < nb; i += blockDim.x) {
            h[i] = __hip_atomic_load(gh + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(gh + i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (HEAD && threadIdx.x < 2) {
            head_n[threadIdx.x] = __hip_atomic_load(ws + kWsHeadV + 2 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ws + kWsHeadV + 2 + threadIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
    int mine = 0;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) {
        const int n = h[i];
        if (i < C) mine += n;
        if (update && n != 0) cum[i] += (float)n;
    }
    if (mine != 0) atomicAdd(&npos, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[2] = npos;
        if (HEAD) { ws[kWsHeadV] = head_n[0]; ws[kWsHeadV + 1] = head_n[1]; }
        if (gridDim.x > 1) __hip_atomic_store(ws + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------------------ loss
struct SeesawArgs {
    const float* x; int64_t ldx;
    const int64_t* labels; const float* roww; const float* cum;
    float p, q, log_eps, scale_cls, scale_obj;
    int div_pos, N, C;
    float* rows_cls; float* rows_obj; float* loss_out;
    float* dx; int64_t lddx;
    int32_t* status; int32_t* ws;
    float loss_weight; float* acc_out; float* avg_out;          // HEAD instances only
};

// One row's class columns in NCH registers per lane (column j * 64 + lane) and one extra dword: lanes 0 / 1 the two objectness
// columns, lane 2 the target's logit (column 0 when the row has no class target).  Every address is inside the row.
// EXACT: C fills every chunk but the last (NCH = ceil(C / 64), the LVIS instance), so only that one is tested; otherwise the
// instance has more chunks than the row and every chunk is.
template <int NCH, bool EXACT>
__device__ __forceinline__ bool seesaw_has_col(int j, int lane, int C) {
    if (EXACT && j < NCH - 1) return true;
    return j * 64 + lane < C;
}

template <int NCH, bool EXACT>
__device__ __forceinline__ void seesaw_load_row(const float* xp, int C, int64_t lab, int lane, float (&dst)[NCH], float& aux) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) dst[j] = xp[seesaw_has_col<NCH, EXACT>(j, lane, C) ? j * 64 + lane : 0];
    const int tcol = (lab >= 0 && lab < C) ? (int)lab : 0;
    aux = xp[lane < 2 ? C + lane : tcol];
}

// The end of a HEAD launch, called by every thread with its wave's sums (wave-uniform): two float sums and two INTEGER hit counts
// reach thread 0 of the last block (loss_reduce.h), which reads the two row counts of the count launch, writes the five results
// and puts the ticket back to zero.
__device__ __forceinline__ void seesaw_head_finish(const SeesawArgs& a, float wave_cls, float wave_obj, int wave_ho, int wave_hc) {
    float sum[2] = {wave_cls, wave_obj};
    int hits[2] = {wave_ho, wave_hc};
    if (!ticketed_sums<2, 2, kHeadThreads>(a.ws, a.ws + kWsHeadPartial, sum, hits)) return;
    const int valid = a.ws[kWsHeadV], npos = a.ws[kWsHeadV + 1];         // of the count launch, earlier on the stream
    const float avg = (float)(valid > 1 ? valid : 1);
    const float lc = a.loss_weight * (sum[0] / avg), lo = a.loss_weight * (sum[1] / avg);
    a.loss_out[0] = lc;
    a.loss_out[1] = lo;
    a.loss_out[2] = lc + lo;                                              // return_dict=False: seesaw_loss.py:261
    // accuracy.py:49-50: float32 hit count times the float32 value of the double 100 / rows; 0 for no rows
    a.acc_out[0] = valid > 0 ? (float)hits[0] * (float)(100.0 / (double)avg) : 0.f;
    a.acc_out[1] = npos > 0 ? (float)hits[1] * (float)(100.0 / (double)npos) : 0.f;
    *a.avg_out = avg;
    __hip_atomic_store(a.ws, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// HEAD (iif_seesaw_head_fwd, the classification half of BBoxHead.loss without its host read): the same row loop with the row's
// WEIGHT prefetched first - a zero weight issues no further load for the row, whose gradient row is zeros and which enters
// nothing; no row losses are stored; the objectness hits of the rows with w > 0 and the class hits of the positive rows with
// w > 0 (seesaw_loss.py:177-197, iif_topk_hits' rank rule on the raw scores) are counted; and the last block divides by
// avg = max(#{w > 0}, 1), which the count launch left in the workspace.  The two row losses are formed from the same exponentials
// in the forms that do not cancel on a confident row (see the row loop); the gradient is untouched.  The entry passes scale_cls = scale_obj = 1 and
// div_pos = 0, so dscore is at unit scale.  The HEAD = false instances are the code that they were before the parameter.
template <int NCH, bool EXACT, bool HEAD>
__global__ void __launch_bounds__(256) seesaw_loss_kernel(SeesawArgs a) {
    // log(max(cum, 1)); 0 beyond C.  aligned(32), more than any other array of the block asks for, puts it FIRST in LDS: behind the
    // reduction's arrays <4, false, true> takes 65 VGPRs for 62 and loses a wave per SIMD
    __shared__ __attribute__((aligned(32))) float lc_s[NCH * 64];
    const int lane = threadIdx.x & 63;
    const int wpb = block_threads() >> 6;              // read here, it is at hand for the reduction at the end (loss_reduce.h)
    const int nwaves = gridDim.x * wpb;
    int row = __builtin_amdgcn_readfirstlane(blockIdx.x * wpb + (threadIdx.x >> 6));
    float xn[NCH], auxn = 0.f;
    int64_t labn = 0;
    float wn = 0.f;                                    // HEAD: the weight of the row in xn
    if (row < a.N) {                                   // in flight while the table is staged
        if (HEAD) wn = a.roww ? a.roww[row] : 1.0f;
        if (!HEAD || wn != 0.f) {
            labn = a.labels[row];
            seesaw_load_row<NCH, EXACT>(a.x + (int64_t)row * a.ldx, a.C, labn, lane, xn, auxn);
        }
    }
#pragma unroll
    for (int k = 0; k < (NCH * 64 + 255) / 256; ++k) {
        const int i = threadIdx.x + k * 256;
        if (i < NCH * 64) lc_s[i] = i < a.C ? kLn2 * fast_log2(fmaxf(a.cum[i], 1.0f)) : 0.f;
    }
    // positives of this call, written by the count launch; 'mean' without avg_factor divides the class loss by it
    float sc = a.scale_cls;
    if (a.div_pos) {
        const int npos = a.ws[2];
        sc = npos > 0 ? a.scale_cls / (float)npos : 0.f;
    }
    __syncthreads();
    float wave_cls = 0.f, wave_obj = 0.f;
    int wave_ho = 0, wave_hc = 0;                      // HEAD: objectness and class hits (wave-uniform)
    for (; row < a.N; row += nwaves) {
        asm volatile("" ::: "memory");                 // keep the table reads in LDS
        float z[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) z[j] = seesaw_has_col<NCH, EXACT>(j, lane, a.C) ? xn[j] : -INFINITY;
        const float aux = auxn;
        const int64_t lab = labn;
        const float wrow = wn;
        // the next row's loads go out before this row's stores (vmcnt retires in order)
        const int nrow = row + nwaves;
        if (nrow < a.N) {
            if (HEAD) wn = a.roww ? a.roww[nrow] : 1.0f;
            if (!HEAD || wn != 0.f) {
                labn = a.labels[nrow];
                seesaw_load_row<NCH, EXACT>(a.x + (int64_t)nrow * a.ldx, a.C, labn, lane, xn, auxn);
            }
        }
        if (HEAD && wrow == 0.f) {                     // wave-uniform: nothing of the row was read
            if (a.dx) {
                float* dz = a.dx + (int64_t)row * a.lddx;
#pragma unroll
                for (int j = 0; j < NCH; ++j)
                    if (seesaw_has_col<NCH, EXACT>(j, lane, a.C)) dz[j * 64 + lane] = 0.f;
                if (lane < 2) dz[a.C + lane] = 0.f;
            }
            continue;
        }
        const bool valid = lab >= 0 && lab <= a.C;
        const bool pos = valid && lab < a.C;
        const int t = pos ? (int)lab : -1;
        if (!valid && a.status && lane == 0) atomicExch(a.status, 1);
        const float w = valid ? (HEAD ? wrow : a.roww ? a.roww[row] : 1.0f) : 0.0f;      // an out-of-range label zeroes its row
        float* dx = a.dx ? a.dx + (int64_t)row * a.lddx : nullptr;
        // objectness: two columns, label (lab == C)
        {
            const float o0 = __shfl(aux, 0, 64), o1 = __shfl(aux, 1, 64);
            const float mo = fmaxf(o0, o1);
            const float e0 = fast_exp2((o0 - mo) * kLog2e), e1 = fast_exp2((o1 - mo) * kLog2e);
            const float so = e0 + e1;
            const bool neg = lab == a.C;
            // HEAD: the two-column cross entropy is softplus(other - target), which does not cancel on a confident row
            // (mo + log(so) - target is right only to ulp(mo), more than such a row's whole loss); the gradient is the same
            const float lo = !valid ? 0.f
                           : HEAD ? w * sigmoid_elem(neg ? o0 - o1 : o1 - o0).spp
                                  : w * (mo + kLn2 * fast_log2(so) - (neg ? o1 : o0));
            wave_obj += lo;
            if (!HEAD && lane == 0) a.rows_obj[row] = lo;
            if (HEAD) {                                // a hit: the other column neither greater nor equal at a lower index
                const float ot = neg ? o1 : o0, oo = neg ? o0 : o1;
                wave_ho += valid && wrow > 0.f && !((oo > ot) || (oo == ot && neg));
            }
            if (dx && lane < 2) {
                const float g = a.scale_obj * w;
                const float pr = (lane == 0 ? e0 : e1) / so;
                dx[a.C + lane] = valid ? g * (pr - ((lane == 1) == neg ? 1.0f : 0.0f)) : 0.f;
            }
        }
        if (!pos) {                                    // wave-uniform: background rows have no class loss and no class gradient
            if (!HEAD && lane == 0) a.rows_cls[row] = 0.f;
            if (dx) {
#pragma unroll
                for (int j = 0; j < NCH; ++j)
                    if (seesaw_has_col<NCH, EXACT>(j, lane, a.C)) dx[j * 64 + lane] = 0.f;
            }
            continue;
        }
        // first softmax: lse(z), for the compensation term
        const float zt = __shfl(aux, 2, 64);
        if (HEAD && wrow > 0.f) {                      // wave-uniform; on the raw scores, before the seesaw terms go in
            int c = 0;
#pragma unroll
            for (int j = 0; j < NCH; ++j) c += (z[j] > zt) || (z[j] == zt && j * 64 + lane < t);
            wave_hc += wave_sum_i(c) == 0;
        }
        float base = 0.f;
        if (a.q > 0.f) {
            float m = z[0];
#pragma unroll
            for (int j = 1; j < NCH; ++j) m = fmaxf(m, z[j]);
            m = wave_max(m);
            const float m2 = m * kLog2e;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j) s += fast_exp2(__builtin_fmaf(z[j], kLog2e, -m2));
            s = wave_sum(s);
            const float lse = m + kLn2 * fast_log2(s);
            base = lse + fmaxf(zt - lse, a.log_eps);   // log of the clamped target score, plus lse
        }
        const float lct = lc_s[t];
        float mm = -INFINITY;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int col = j * 64 + lane;
            float add = 0.f;
            if (a.p > 0.f) add += fminf(0.f, a.p * (lc_s[col] - lct));     // mitigation: rarer classes are pushed less
            if (a.q > 0.f) add += fmaxf(0.f, a.q * (z[j] - base));         // compensation: confident mistakes are pushed more
            if (col != t) z[j] += add;
            mm = fmaxf(mm, z[j]);
        }
        mm = wave_max(mm);
        const float mm2 = mm * kLog2e;
        float s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            z[j] = fast_exp2(__builtin_fmaf(z[j], kLog2e, -mm2));
            s2 += z[j];
        }
        s2 = wave_sum(s2);
        float lc = w * (mm + kLn2 * fast_log2(s2) - zt);
        if constexpr (HEAD) {
            // the same value with the target's own term e_t kept out of the sum, as head_loss.hip does it:
            // lse(z') - z_t = log1p(sum_{j != t} e_j / e_t), which has nothing to cancel on a confident hit.  Every e_j carries
            // the same factor 2^(mm log2 e - mm2), which the quotient drops.  (e_t underflows only for a target ~87 below the
            // maximum, where the form above has nothing to cancel either.)
            float so = 0.f, et = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const bool tgt = j * 64 + lane == t;
                so += tgt ? 0.f : z[j];
                et += tgt ? z[j] : 0.f;
            }
            so = wave_sum(so);
            et = wave_sum(et);
            if (et > 1e-30f) lc = w * log1pf(so / et);
        }
        wave_cls += lc;
        if (!HEAD && lane == 0) a.rows_cls[row] = lc;
        if (dx) {
            const float g = sc * w, gs = g / s2;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int col = j * 64 + lane;
                if (seesaw_has_col<NCH, EXACT>(j, lane, a.C)) dx[col] = z[j] * gs - (col == t ? g : 0.f);
            }
        }
    }
    // both scalar losses out of the same launch (loss_reduce.h): ticket at ws[0], interleaved cls / obj partials, under HEAD
    // with the two hit counts behind them
    if constexpr (!HEAD) {
        ticketed_finish<2>(a.ws, {wave_cls, wave_obj}, {sc, a.scale_obj}, {a.loss_out, a.loss_out + 1}, kWsPartial);
    } else {
        seesaw_head_finish(a, wave_cls, wave_obj, wave_ho, wave_hc);
    }
}

// ------------------------------------------------------------------------------------------------ activation
// out[:, :C] = softmax(z) * softmax(o)[0], out[:, C] = softmax(o)[1]
template <int NCH, bool EXACT>
__global__ void __launch_bounds__(256) seesaw_activation_kernel(const float* x, int64_t ldx, int N, int C, float* out, int64_t ldo) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
        float z[NCH], aux;
        seesaw_load_row<NCH, EXACT>(x + (int64_t)row * ldx, C, -1, lane, z, aux);
#pragma unroll
        for (int j = 0; j < NCH; ++j)
            if (!seesaw_has_col<NCH, EXACT>(j, lane, C)) z[j] = -INFINITY;
        const float o0 = __shfl(aux, 0, 64), o1 = __shfl(aux, 1, 64);
        const float mo = fmaxf(o0, o1);
        const float e0 = fast_exp2((o0 - mo) * kLog2e), e1 = fast_exp2((o1 - mo) * kLog2e);
        const float inv_o = 1.0f / (e0 + e1);
        float m = z[0];
#pragma unroll
        for (int j = 1; j < NCH; ++j) m = fmaxf(m, z[j]);
        m = wave_max(m);
        const float m2 = m * kLog2e;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            z[j] = fast_exp2(__builtin_fmaf(z[j], kLog2e, -m2));
            s += z[j];
        }
        s = wave_sum(s);
        const float f = (e0 * inv_o) / s;
        float* o = out + (int64_t)row * ldo;
#pragma unroll
        for (int j = 0; j < NCH; ++j)
            if (seesaw_has_col<NCH, EXACT>(j, lane, C)) o[j * 64 + lane] = z[j] * f;
        if (lane == 0) o[C] = e1 * inv_o;
    }
}

// ------------------------------------------------------------------------------------------------ accuracy
// ws: int32[4] = ticket, objectness hits, class hits, positive rows (zero between calls).  Rank rule of iif_topk_hits:
// a row is a hit when no column is greater than the target's and no equal one has a lower index.
__global__ void __launch_bounds__(256) seesaw_accuracy_kernel(const float* x, int64_t ldx, const int64_t* labels, int N, int C,
                                                              float* out, int32_t* ws) {
    __shared__ int cnt[3];
    __shared__ int last;
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    __syncthreads();
    int hit_o = 0, hit_c = 0, npos = 0;
    for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
        const float* xr = x + (int64_t)row * ldx;
        const int64_t lab = labels[row];
        const int ol = lab == C ? 1 : 0;
        const float ot = xr[C + ol], oo = xr[C + 1 - ol];
        hit_o += !((oo > ot) || (oo == ot && ol == 1));
        if (lab < 0 || lab >= C) continue;             // wave-uniform
        const int t = (int)lab;
        const float zt = xr[t];
        int c = 0;
        for (int col = lane; col < C; col += 64) {
            const float z = xr[col];
            c += (z > zt) || (z == zt && col < t);
        }
        c = wave_sum_i(c);
        hit_c += c == 0;
        npos += 1;
    }
    if (lane == 0) {
        if (hit_o) atomicAdd(&cnt[0], hit_o);
        if (hit_c) atomicAdd(&cnt[1], hit_c);
        if (npos) atomicAdd(&cnt[2], npos);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int back = 0;
        for (int k = 0; k < 3; ++k) back += __hip_atomic_fetch_add(ws + 1 + k, cnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" : : "v"(back) : "memory");
        const int tk = __hip_atomic_fetch_add(ws, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (tk == (int)gridDim.x - 1);
        if (last) {
            int v[3];
            for (int k = 0; k < 3; ++k) {
                v[k] = __hip_atomic_load(ws + 1 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ws + 1 + k, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // accuracy.py:49-50: float32 hit count times the float32 value of the double 100 / rows; 0 for no rows
            out[0] = (float)v[0] * (float)(100.0 / (double)N);
            out[1] = v[2] > 0 ? (float)v[1] * (float)(100.0 / (double)v[2]) : 0.f;
            __hip_atomic_store(ws, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward scaling
// out = d * (g_cls on the class columns, g_obj on the two objectness columns); the upstream values are device scalars
// (per_row == 0) or one value per row (reduction='none')
__global__ void __launch_bounds__(256) seesaw_scale_grad_kernel(const float* d, int64_t ld, int N, int C, const float* g_cls,
                                                                const float* g_obj, int per_row, float* out, int64_t ldo) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
        const float gc = g_cls[per_row ? row : 0], go = g_obj[per_row ? row : 0];
        const float* dr = d + (int64_t)row * ld;
        float* o = out + (int64_t)row * ldo;
        for (int col = lane; col < C + 2; col += 64) o[col] = dr[col] * (col < C ? gc : go);
    }
}

// backward of iif_seesaw_head_fwd: out = d * (g_cls * loss_weight / avg) on the class columns and d * (g_obj * loss_weight / avg)
// on the two objectness columns, every factor a device scalar
__global__ void __launch_bounds__(256) seesaw_head_scale_kernel(const float* d, int64_t ld, int N, int C, const float* g_cls,
                                                                const float* g_obj, const float* avg, float loss_weight, float* out,
                                                                int64_t ldo) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const float gc = (*g_cls * loss_weight) / *avg, go = (*g_obj * loss_weight) / *avg;
    for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
        const float* dr = d + (int64_t)row * ld;
        float* o = out + (int64_t)row * ldo;
        for (int col = lane; col < C + 2; col += 64) o[col] = dr[col] * (col < C ? gc : go);
    }
}

inline unsigned row_grid(int N, unsigned maxb) {
    const unsigned g = (unsigned)((N + 3) / 4);
    return g < maxb ? g : maxb;
}

// chunks of 64 class columns -> the instantiated chunk count at or above it; exact when they are equal
#define SEESAW_PICK(nch, K, CALL)                        \
    do {                                                 \
        if ((nch) == (K)) { CALL(K, true); }             \
        else { CALL(K, false); }                         \
    } while (0)
#define SEESAW_DISPATCH(nch, CALL)                                  \
    do {                                                            \
        if ((nch) <= 1) SEESAW_PICK(nch, 1, CALL);                  \
        else if ((nch) <= 2) SEESAW_PICK(nch, 2, CALL);             \
        else if ((nch) <= 4) SEESAW_PICK(nch, 4, CALL);             \
        else if ((nch) <= 8) SEESAW_PICK(nch, 8, CALL);             \
        else if ((nch) <= 12) SEESAW_PICK(nch, 12, CALL);           \
        else if ((nch) <= 16) SEESAW_PICK(nch, 16, CALL);           \
        else if ((nch) <= 19) SEESAW_PICK(nch, 19, CALL); /* LVIS */ \
        else if ((nch) <= 24) SEESAW_PICK(nch, 24, CALL);           \
        else SEESAW_PICK(nch, 32, CALL);                            \
    } while (0)

}  // namespace

extern "C" {

int iif_seesaw_fwd_bwd(const void* cls_score, int dtype, int64_t ld_score, const int64_t* labels, const float* label_weights,
                       float* cum_samples, int update_counts, float p, float q, float eps, float scale_cls, int div_by_pos,
                       float scale_obj, int N, int C, float* loss_rows_cls, float* loss_rows_obj, float* loss_out,
                       void* dscore, int64_t ld_dscore, int32_t* d_status, void* d_workspace, void* stream) {
    if (N < 0 || C <= 0) return IIF_EINVAL;
    if (dtype != IIF_F32) return IIF_EINVAL;
    if (!(p >= 0.f) || !(q >= 0.f) || (q > 0.f && !(eps > 0.f))) return IIF_EINVAL;
    if (!loss_out) return IIF_EINVAL;
    if ((int64_t)C + 2 > kMaxCols) return IIF_EUNSUPPORTED;
    hipStream_t st = as_stream(stream);
    if (N == 0) {
        if (hipMemsetAsync(loss_out, 0, 2 * sizeof(float), st) != hipSuccess) return IIF_ELAUNCH;
        return IIF_OK;
    }
    if (!cls_score || !labels || !cum_samples || !loss_rows_cls || !loss_rows_obj || !d_workspace) return IIF_EINVAL;
    if (ld_score < C + 2 || (dscore && ld_dscore < C + 2)) return IIF_EINVAL;
    int32_t* ws = static_cast<int32_t*>(d_workspace);
    int cb = (N + kLabelsPerCountBlock - 1) / kLabelsPerCountBlock;
    if (cb > kMaxCountBlocks) cb = kMaxCountBlocks;
    hipLaunchKernelGGL(seesaw_count_kernel<false>, dim3(cb), dim3(kCountBlock), 0, st, labels, (const float*)nullptr, N, C, cum_samples,
                       update_counts, ws, d_status);
    IIF_LAUNCH_CHECK();
    SeesawArgs a{static_cast<const float*>(cls_score), ld_score, labels, label_weights, cum_samples, p, q,
                 q > 0.f ? logf(eps) : 0.f, scale_cls, scale_obj, div_by_pos, N, C, loss_rows_cls, loss_rows_obj, loss_out,
                 static_cast<float*>(dscore), ld_dscore, d_status, ws, 0.f, nullptr, nullptr};
    // 512 blocks of four waves: beyond that a wave walks several rows (iif_head.hip measured the same grid for fp32 rows)
    const dim3 grid(row_grid(N, 512)), block(256);
    static_assert(512 <= kMaxLossBlocks, "one partial slot per block");
    const int nch = (C + 63) / 64;
#define CALL(K, E) hipLaunchKernelGGL((seesaw_loss_kernel<K, E, false>), grid, block, 0, st, a)
    SEESAW_DISPATCH(nch, CALL);
#undef CALL
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_seesaw_head_fwd(const void* cls_score, int dtype, int64_t ld_score, const int64_t* labels, const float* label_weights,
                        float* cum_samples, float p, float q, float eps, float loss_weight, int N, int C, void* dscore,
                        int64_t ld_dscore, float* loss_out, float* acc_out, float* avg_out, int32_t* d_status, void* d_workspace,
                        void* stream) {
    if (N < 0 || N > IIF_HEAD_LOSS_MAX_ROWS || C <= 0) return IIF_EINVAL;
    if (dtype != IIF_F32) return IIF_EINVAL;
    if (!(p >= 0.f) || !(q >= 0.f) || (q > 0.f && !(eps > 0.f))) return IIF_EINVAL;
    if (!loss_out || !acc_out || !avg_out || !cum_samples || !d_workspace) return IIF_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_workspace) % 4 != 0 || reinterpret_cast<uintptr_t>(cls_score) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(dscore) % 4 != 0)
        return IIF_EINVAL;
    if (N > 0 && (!cls_score || !labels)) return IIF_EINVAL;
    if (N > 0 && (ld_score < (int64_t)C + 2 || (dscore && ld_dscore < (int64_t)C + 2))) return IIF_EINVAL;
    if ((int64_t)C + 2 > kMaxCols) return IIF_EUNSUPPORTED;
    hipStream_t st = as_stream(stream);
    int32_t* ws = static_cast<int32_t*>(d_workspace);
    int cb = (N + kLabelsPerCountBlock - 1) / kLabelsPerCountBlock;
    if (cb < 1) cb = 1;                                // N == 0: one block of each launch, for loss 0, acc 0, avg 1
    hipLaunchKernelGGL(seesaw_count_kernel<true>, dim3(cb), dim3(kCountBlock), 0, st, labels, label_weights, N, C, cum_samples, 1, ws,
                       d_status);
    IIF_LAUNCH_CHECK();
    SeesawArgs a{static_cast<const float*>(cls_score), ld_score, labels, label_weights, cum_samples, p, q,
                 q > 0.f ? logf(eps) : 0.f, 1.0f, 1.0f, 0, N, C, nullptr, nullptr, loss_out,
                 N > 0 ? static_cast<float*>(dscore) : nullptr, ld_dscore, d_status, ws, loss_weight, acc_out, avg_out};
    unsigned g = row_grid(N, 512);
    if (g < 1) g = 1;
    const dim3 grid(g), block(kHeadThreads);
    const int nch = (C + 63) / 64;
#define CALL(K, E) hipLaunchKernelGGL((seesaw_loss_kernel<K, E, true>), grid, block, 0, st, a)
    SEESAW_DISPATCH(nch, CALL);
#undef CALL
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_seesaw_head_bwd(const float* dscore, int64_t ld_dscore, int N, int C, const float* d_g_cls, const float* d_g_obj,
                        const float* d_avg, float loss_weight, float* out, int64_t ld_out, void* stream) {
    if (N < 0 || C <= 0 || !d_g_cls || !d_g_obj || !d_avg) return IIF_EINVAL;
    if (N == 0) return IIF_OK;
    if (!dscore || !out || ld_dscore < (int64_t)C + 2 || ld_out < (int64_t)C + 2) return IIF_EINVAL;
    if (reinterpret_cast<uintptr_t>(dscore) % 4 != 0 || reinterpret_cast<uintptr_t>(out) % 4 != 0) return IIF_EINVAL;
    hipLaunchKernelGGL(seesaw_head_scale_kernel, dim3(row_grid(N, 2048)), dim3(256), 0, as_stream(stream), dscore, ld_dscore, N, C,
                       d_g_cls, d_g_obj, d_avg, loss_weight, out, ld_out);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_seesaw_activation(const void* cls_score, int dtype, int64_t ld_score, int N, int C, float* out, int64_t ld_out,
                          void* stream) {
    if (N < 0 || C <= 0) return IIF_EINVAL;
    if (dtype != IIF_F32) return IIF_EINVAL;
    if ((int64_t)C + 2 > kMaxCols) return IIF_EUNSUPPORTED;
    if (N == 0) return IIF_OK;
    if (!cls_score || !out || ld_score < C + 2 || ld_out < C + 1) return IIF_EINVAL;
    const dim3 grid(row_grid(N, 2048)), block(256);
    const float* x = static_cast<const float*>(cls_score);
    const int nch = (C + 63) / 64;
#define CALL(K, E) hipLaunchKernelGGL((seesaw_activation_kernel<K, E>), grid, block, 0, as_stream(stream), x, ld_score, N, C, out, ld_out)
    SEESAW_DISPATCH(nch, CALL);
#undef CALL
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_seesaw_accuracy(const void* cls_score, int dtype, int64_t ld_score, const int64_t* labels, int N, int C, float* out,
                        int32_t* d_workspace, void* stream) {
    if (N < 0 || C <= 0 || !out) return IIF_EINVAL;
    if (dtype != IIF_F32) return IIF_EINVAL;
    hipStream_t st = as_stream(stream);
    if (N == 0) {
        if (hipMemsetAsync(out, 0, 2 * sizeof(float), st) != hipSuccess) return IIF_ELAUNCH;
        return IIF_OK;
    }
    if (!cls_score || !labels || !d_workspace || ld_score < C + 2) return IIF_EINVAL;
    hipLaunchKernelGGL(seesaw_accuracy_kernel, dim3(row_grid(N, 1024)), dim3(256), 0, st, static_cast<const float*>(cls_score),
                       ld_score, labels, N, C, out, d_workspace);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int iif_seesaw_scale_grad(const float* dscore, int64_t ld_dscore, int N, int C, const float* g_cls, const float* g_obj,
                          int per_row, float* out, int64_t ld_out, void* stream) {
    if (N < 0 || C <= 0) return IIF_EINVAL;
    if (N == 0) return IIF_OK;
    if (!dscore || !g_cls || !g_obj || !out || ld_dscore < C + 2 || ld_out < C + 2) return IIF_EINVAL;
    hipLaunchKernelGGL(seesaw_scale_grad_kernel, dim3(row_grid(N, 2048)), dim3(256), 0, as_stream(stream), dscore, ld_dscore, N,
                       C, g_cls, g_obj, per_row, out, ld_out);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // extern "C"
