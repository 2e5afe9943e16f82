// Evaluation statistics of a classifier head for gfx950 (MI355X): top-k hits, per-class test / hit counts (the
// many / median / low-shot split) and reliability bins (ECE / MCE), accumulated on the device in ONE launch per batch.
//
// One 64-lane wave owns one row of z = x * table (fp32 products, what iif_scale_logits stores) and reads it once:
//   * rank of the target = #greater + #equal-with-lower-index (iif_topk_hits's rule, so the hits are bit-equal);
//   * prediction = the first index of the maximum (torch.argmax); the wave reduction breaks ties by the smaller index;
//   * confidence = the softmax maximum 1 / sum exp(z_c - z_max): every lane sums 2^((z - m_lane) log2 e) against its own
//     maximum, the wave rescales the lane sums to the row maximum (online max / rescaled sum, base-2 v_exp_f32 as the IIF
//     head).  The difference z - m is formed before the scaling, so the maximum contributes exactly 1 and conf <= 1;
//   * bins: np.digitize(conf, edges, right=True): bin b holds edges[b] < (double)conf <= edges[b + 1] with the caller's
//     float64 edges, a value outside (edges[0], edges[nb]] (NaN included) lands in no bin.
// Accumulation is integer only: per-block LDS partials (int64) for the rows / out-of-range / top-k / bin slots, flushed
// with one global atomic per non-zero slot per block; n_test[t] / n_hit[t] take one global atomic per row.  The
// confidence enters bin_conf as the fixed-point llrint(conf * 2^32), so every sum is exact and independent of the launch
// order, the batch split and the rank count.  No float atomics (cdna_hip_programming.md Guideline 12).
// A row whose target lies outside [0, C) counts in rows, out_of_range and the bins (as a miss) and in no per-class slot.
// Logits holding NaN: NaN compares false, so the prediction is the first maximum of the other values and conf is NaN.
#include <limits.h>

#include "common.h"
#include "head_math.h"
#include "vec16.h"

namespace {

constexpr int kMaxBins = 256;
constexpr int kWpb = 4;                       // waves per block
// rows beyond 4 x kMaxBlocks are walked by the same waves (fewer block flushes).  Measured at [65536, 1000] fp32 with a table:
// 512 / 1024 / 2048 / 8192 blocks = 101 / 66 / 69 / 121 us (too few rows in flight / the flush atomics on the shared slots)
constexpr unsigned kMaxBlocks = 1024;
constexpr int kSlots = 6;                     // LDS: rows, out_of_range, hits[4], then 3 x nb bin slots


struct EvalArgs {
    const void* x; int64_t ldx;
    const float* tab;
    const int64_t* tgt;
    int B, C;
    int k[4]; int nk;
    const double* edges; int nb;
    int64_t* acc;
    int64_t* pred_out; float* conf_out;
};

__device__ __forceinline__ void lds_add(long long* p, long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void gl_add(int64_t* p, long long v) {
    __hip_atomic_fetch_add(reinterpret_cast<long long*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// block prologue: zero the LDS partials, stage the bin edges
__device__ __forceinline__ void block_begin(const EvalArgs& a, long long* s, double* e) {
    for (int i = threadIdx.x; i < kSlots + 3 * a.nb; i += blockDim.x) s[i] = 0;
    for (int i = threadIdx.x; i <= a.nb; i += blockDim.x) e[i] = a.edges[i];
    __syncthreads();
}

// block epilogue: one global atomic per non-zero slot
__device__ __forceinline__ void block_end(const EvalArgs& a, const long long* s) {
    __syncthreads();
    const int nh = 2 + a.nk, nbin = 3 * a.nb;
    for (int i = threadIdx.x; i < nh + nbin; i += blockDim.x) {
        const long long v = i < nh ? s[i] : s[kSlots + i - nh];
        const int64_t off = i < nh ? i : (int64_t)nh + 2 * (int64_t)a.C + (i - nh);
        if (v != 0) gl_add(a.acc + off, v);
    }
}

// Wave-wide first maximum and the row's softmax sum from per-lane (max, first index of it, sum relative to that max).
__device__ __forceinline__ void wave_finish(float& m, int& idx, float& s) {
    const float ml = m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (om > m || (om == m && oi < idx)) { m = om; idx = oi; }
    }
    s = ml == -INFINITY ? 0.f : s * fast_exp2((ml - m) * kLog2e);
    s = wave_sum(s);
}

// Per-row bookkeeping; called by the whole wave with wave-uniform values, lane 0 writes.
__device__ __forceinline__ void finish_row(const EvalArgs& a, long long* s, const double* e, int row, int64_t t,
                                           int rank, int pred, float conf) {
    if ((threadIdx.x & 63) != 0) return;
    lds_add(s + 0, 1);
    const bool ok = t >= 0 && t < a.C;
    const bool hit = ok && pred == (int)t;
    if (!ok) {
        lds_add(s + 1, 1);
    } else {
        for (int j = 0; j < a.nk; ++j)
            if (rank < a.k[j]) lds_add(s + 2 + j, 1);
        gl_add(a.acc + 2 + a.nk + t, 1);
        if (hit) gl_add(a.acc + 2 + a.nk + a.C + t, 1);
    }
    const double c = (double)conf;
    if (c > e[0] && c <= e[a.nb]) {                      // e[lo] < c <= e[hi]
        int lo = 0, hi = a.nb;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (c <= e[mid]) hi = mid; else lo = mid;
        }
        long long* sb = s + kSlots;
        lds_add(sb + lo, 1);
        if (hit) lds_add(sb + a.nb + lo, 1);
        lds_add(sb + 2 * a.nb + lo, (long long)rintf(conf * 4294967296.0f));     // exact: conf * 2^32 < 2^33
    }
    if (a.pred_out) a.pred_out[row] = pred;
    if (a.conf_out) a.conf_out[row] = conf;
}

// ------------------------------------------------------------- row in registers (C % 4 == 0, C <= 2048)
// One lane holds V consecutive columns per chunk: 16 bytes of fp32 (4) or bf16 (8); a bf16 row with C % 8 == 4 ends on
// an 8-byte half vector in some lane.  Only the last chunk (NCH - 1) can be ragged.  The lane's table entries are loop
// invariant and stay in registers; the next row's loads are issued before the current row is reduced.

template <typename T, int NCH, bool TAB>
__global__ void __launch_bounds__(256) eval_reg_kernel(EvalArgs a) {
    constexpr int V = VT<T>::V;
    constexpr int JL = NCH - 1;
    __shared__ long long s_acc[kSlots + 3 * kMaxBins];
    __shared__ double s_edges[kMaxBins + 1];
    const int lane = threadIdx.x & 63;
    const int nwaves = gridDim.x * kWpb;
    int row = blockIdx.x * kWpb + (threadIdx.x >> 6);
    const int left = a.C - (JL * 64 + lane) * V;        // columns of the last chunk this lane owns: V, 4 (bf16) or 0
    const int nl = left >= V ? V : (left > 0 ? left : 0);
    typename VT<T>::Raw xr[NCH];
    auto load_row = [&](int r) {
        const T* xp = static_cast<const T*>(a.x) + (int64_t)r * a.ldx;
#pragma unroll
        for (int j = 0; j < JL; ++j) xr[j] = VT<T>::raw_row(xp + (j * 64 + lane) * V, V);
        xr[JL] = VT<T>::raw_row(xp + (JL * 64 + lane) * V, nl);
    };
    if (row < a.B) load_row(row);                     // wave-uniform; in flight while the block stages its LDS
    float tb[NCH][V];
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int q = 0; q < V; q += 4) {
            f32x4 t4 = f32x4{1.f, 1.f, 1.f, 1.f};
            if (TAB && (j < JL || q < nl)) t4 = *reinterpret_cast<const f32x4*>(a.tab + (j * 64 + lane) * V + q);
            tb[j][q] = t4.x; tb[j][q + 1] = t4.y; tb[j][q + 2] = t4.z; tb[j][q + 3] = t4.w;
        }
    block_begin(a, s_acc, s_edges);
    const int first_col = lane * V < a.C ? lane * V : INT_MAX;
    for (; row < a.B; row += nwaves) {
        const int64_t t = a.tgt[__builtin_amdgcn_readfirstlane(row)];
        float z[NCH][V];
        float m = -INFINITY;
        int mi = first_col;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            float xv[V];
            VT<T>::unpack(xr[j], xv);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const bool valid = j < JL || e < nl;
                z[j][e] = valid ? (TAB ? xv[e] * tb[j][e] : xv[e]) : -INFINITY;
                if (z[j][e] > m) { m = z[j][e]; mi = (j * 64 + lane) * V + e; }
            }
        }
        if (row + nwaves < a.B) load_row(row + nwaves);   // wave-uniform
        // the target's product out of the owning lane's registers (chunk, lane and element are wave-uniform)
        const bool ok = t >= 0 && t < a.C;
        const int ti = ok ? (int)t : 0;
        const int tj = ti / (64 * V), tl = (ti / V) & 63, te = ti % V;
        float zt = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j)
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (tj == j && te == e) zt = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, z[j][e]), tl));
        int cnt = 0;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j)
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int c = (j * 64 + lane) * V + e;          // >= C where the column does not exist (c < t is false)
                cnt += (z[j][e] > zt) | ((z[j][e] == zt) & (c < ti));
                s += fast_exp2((z[j][e] - m) * kLog2e);        // -inf -> 0; the lane maximum -> exactly 1
            }
        cnt = wave_sum_i(cnt);
        wave_finish(m, mi, s);
        finish_row(a, s_acc, s_edges, row, t, cnt, mi, 1.0f / s);
    }
    block_end(a, s_acc);
}

// ------------------------------------------------------------- streaming row (any C, any alignment)
template <typename T, bool TAB>
__global__ void __launch_bounds__(256) eval_stream_kernel(EvalArgs a) {
    __shared__ long long s_acc[kSlots + 3 * kMaxBins];
    __shared__ double s_edges[kMaxBins + 1];
    block_begin(a, s_acc, s_edges);
    const int lane = threadIdx.x & 63;
    const int nwaves = gridDim.x * kWpb;
    for (int row = blockIdx.x * kWpb + (threadIdx.x >> 6); row < a.B; row += nwaves) {
        const T* x = static_cast<const T*>(a.x) + (int64_t)row * a.ldx;
        const int64_t t = a.tgt[row];
        const bool ok = t >= 0 && t < a.C;
        const float zt = ok ? VT<T>::load1(x + t) * (TAB ? a.tab[t] : 1.0f) : 0.f;
        float m = -INFINITY, s = 0.f;
        int mi = lane < a.C ? lane : INT_MAX, cnt = 0;
        for (int c = lane; c < a.C; c += 64) {
            const float z = VT<T>::load1(x + c) * (TAB ? a.tab[c] : 1.0f);
            cnt += (z > zt) | ((z == zt) & (c < (int)t));
            if (z > m) {
                s = s * fast_exp2((m - z) * kLog2e) + 1.0f;
                m = z; mi = c;
            } else if (z != -INFINITY) {
                s += fast_exp2((z - m) * kLog2e);
            }
        }
        cnt = wave_sum_i(cnt);
        wave_finish(m, mi, s);
        finish_row(a, s_acc, s_edges, row, t, cnt, mi, 1.0f / s);
    }
    block_end(a, s_acc);
}

template <typename T, int NCH>
void launch_reg(const EvalArgs& a, dim3 grid, hipStream_t st) {
    if (a.tab) hipLaunchKernelGGL((eval_reg_kernel<T, NCH, true>), grid, dim3(64 * kWpb), 0, st, a);
    else hipLaunchKernelGGL((eval_reg_kernel<T, NCH, false>), grid, dim3(64 * kWpb), 0, st, a);
}

template <typename T>
int launch(const EvalArgs& a, hipStream_t st) {
    const unsigned want = (unsigned)((a.B + kWpb - 1) / kWpb);
    const dim3 grid(want < kMaxBlocks ? want : kMaxBlocks);
    constexpr int V = VT<T>::V;
    constexpr int PA = sizeof(T) == 2 ? 8 : 16;                 // row start alignment in bytes (4 elements)
    const bool reg = a.C % 4 == 0 && a.C <= 2048 && a.ldx % 4 == 0 && aligned(a.x, PA) && (!a.tab || aligned(a.tab, 16));
    if (reg) {
        const int nch = (a.C + 64 * V - 1) / (64 * V);
        switch (nch) {
            case 1: launch_reg<T, 1>(a, grid, st); break;
            case 2: launch_reg<T, 2>(a, grid, st); break;
            case 3: launch_reg<T, 3>(a, grid, st); break;
            case 4: launch_reg<T, 4>(a, grid, st); break;
            default:
                if constexpr (V == 4) {
                    if (nch == 5) launch_reg<T, 5>(a, grid, st);
                    else if (nch == 6) launch_reg<T, 6>(a, grid, st);
                    else if (nch == 7) launch_reg<T, 7>(a, grid, st);
                    else launch_reg<T, 8>(a, grid, st);
                } else {
                    return IIF_EUNSUPPORTED;        // unreachable: C <= 2048 is at most 4 chunks of 512 bf16 columns
                }
        }
    } else if (a.tab) {
        hipLaunchKernelGGL((eval_stream_kernel<T, true>), grid, dim3(64 * kWpb), 0, st, a);
    } else {
        hipLaunchKernelGGL((eval_stream_kernel<T, false>), grid, dim3(64 * kWpb), 0, st, a);
    }
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // namespace

extern "C" int iif_eval_accumulate(const void* logits, int dtype, int64_t ld_logits, const float* table,
                                   const int64_t* targets, int B, int C, const int32_t* k_host, int nk,
                                   const double* bin_edges, int nb, int64_t* acc,
                                   int64_t* pred_out, float* conf_out, void* stream) {
    if (B < 0 || C <= 0 || nk <= 0 || nk > 4 || !k_host || nb < 1 || nb > kMaxBins) return IIF_EINVAL;
    if (dtype != IIF_F32 && dtype != IIF_BF16) return IIF_EINVAL;
    EvalArgs a{};
    for (int j = 0; j < nk; ++j) {
        if (k_host[j] < 1) return IIF_EINVAL;
        a.k[j] = k_host[j];
    }
    if (B == 0) return IIF_OK;
    if (!logits || !targets || !bin_edges || !acc || ld_logits < C) return IIF_EINVAL;
    a.x = logits; a.ldx = ld_logits; a.tab = table; a.tgt = targets; a.B = B; a.C = C; a.nk = nk;
    a.edges = bin_edges; a.nb = nb; a.acc = acc; a.pred_out = pred_out; a.conf_out = conf_out;
    return dtype == IIF_F32 ? launch<float>(a, as_stream(stream)) : launch<unsigned short>(a, as_stream(stream));
}
