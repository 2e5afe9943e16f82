// Fused sigmoid BCE / focal-loss classifier head for gfx950 (MI355X).
//
// classification/custom.py:42-89 (FocalLoss) builds a one-hot target, runs sigmoid + BCELoss (or BCEWithLogitsLoss),
// the modulating factor, the class weights, alpha_t and the reduction as a dozen elementwise launches plus autograd.
// Here ONE launch reads the logits once and writes the per-row loss, the scalar loss and d(loss)/d(logits).
//
// One 64-lane wave walks one row at a time (rows wave_id, wave_id + n_waves, ...).  The elements of a row are
// independent: the only cross-lane work is the row's loss sum, once per row, off the element path.  A row is split into
// a head of < V elements up to the first 16-byte boundary of the logits, a body of 16-byte lane vectors (4 fp32 / 8 bf16
// columns) and a tail of < V elements; head and tail are handled together, one element per lane.  Strided rows, odd
// class counts and unaligned (element-aligned) pointers therefore all take the vector body.  dlogits must share the
// logits' 16-byte phase on every row for that (same address modulo 16, same row pitch modulo 16 bytes); otherwise every
// element goes through the one-per-lane path.
//
// Per element (x = logit; sp(v) = softplus(v), s = sigmoid(x), q = 1 - s: the stable element of head_math.h):
//   gamma == 0:  y=0: l = sp(x),             dl/dx = s
//                y=1: l = sp(-x),            dl/dx = -q
//   gamma  > 0:  y=0: l = s^g sp(x),         dl/dx = s^g (s + g q sp(x))          s^g = exp(-g sp(-x))
//                y=1: l = q^g sp(-x),        dl/dx = -q^g (g s sp(-x) + q)       q^g = exp(-g sp(x))
// gamma 1 and 2 are multiplies.  Three transcendentals per element (the element's), four for other gamma.  Unlike the
// reference (nn.BCELoss clamps log(s) at -100 after s has rounded to 1 in fp32), this is the exact function at every |x|: see
// DESIGN.md, "Sigmoid BCE / focal head".
// Every column is first evaluated as a y = 0 column; the lane(s) owning a target column patch it (mixup: two targets,
// lam * L(y_a) + (1 - lam) * L(y_b) per element).
// The scalar loss comes out of the same launch by the ticketed reduction of loss_reduce.h.
#include "common.h"
#include "head_math.h"
#include "loss_reduce.h"
#include "vec16.h"

namespace {

constexpr int kLdsWeights = 8192;              // class weights staged in LDS up to this many classes (32 KB)

struct Args {
    const void* x; int64_t ldx;
    const int64_t* ta; const int64_t* tb;
    float la, lb;                 // mixup coefficients of the two targets (1, 0 without mixup)
    const float* w;               // class weights [C] or nullptr
    float gamma, a0, a1;          // a0 / a1: alpha_t of y = 0 / y = 1 elements (1 / 1 when off)
    float scale;
    int B, C;
    float* loss_row;
    void* dx; int64_t lddx;
    int32_t* status;
    float* loss_out;
    int32_t* ticket;
    int vec;                      // 1: 16-byte body (launch-level alignment check passed)
};

// y = 0 and y = 1 loss / gradient of one element.  GM: 0 -> gamma 0, 1 / 2 -> gamma 1 / 2, 3 -> any other gamma > 0.
template <int GM>
__device__ __forceinline__ void neg_term(const SigmoidElem& p, float g, float& l, float& d) {      // y = 0
    if constexpr (GM == 0) { l = p.spp; d = p.s; return; }
    const float m = GM == 1 ? p.s : (GM == 2 ? p.s * p.s : exp_neg(g * p.spn));
    l = m * p.spp;
    d = m * (p.s + g * p.q * p.spp);
}

template <int GM>
__device__ __forceinline__ void pos_term(const SigmoidElem& p, float g, float& l, float& d) {      // y = 1
    if constexpr (GM == 0) { l = p.spn; d = -p.q; return; }
    const float m = GM == 1 ? p.q : (GM == 2 ? p.q * p.q : exp_neg(g * p.spp));
    l = m * p.spn;
    d = -m * (g * p.s * p.spn + p.q);
}

// N consecutive columns c0 .. c0 + N - 1 of one row: loss added to acc, gradient (times gs) into d[].
// ta / tb: the row's target columns (-1 when inactive).
// Class weights: w_lds when staged (wsrc 1), a.w in global memory (wsrc 2), none (0); kept apart so that the LDS copy
// is read with ds_read and not through a generic pointer (flat loads wait on both counters).
template <int GM, int N>
__device__ __forceinline__ void columns(const Args& a, int wsrc, const float* w_lds, const float (&x)[N], int c0, int ta,
                                        int tb, float gs, float& acc, float (&d)[N]) {
    SigmoidElem p[N];
    float l[N], w[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
        p[e] = sigmoid_elem(x[e]);
        neg_term<GM>(p[e], a.gamma, l[e], d[e]);
        w[e] = wsrc == 1 ? w_lds[c0 + e] : (wsrc == 2 ? a.w[c0 + e] : 1.0f);
        l[e] *= a.a0;
        d[e] *= a.a0;
    }
    const unsigned da = (unsigned)(ta - c0), db = (unsigned)(tb - c0);
    if ((da < (unsigned)N) | (db < (unsigned)N)) {            // only the lane(s) owning a target column
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const float k = (da == (unsigned)e ? a.la : 0.0f) + (db == (unsigned)e ? a.lb : 0.0f);
            if (k != 0.0f) {
                float l1, d1;
                pos_term<GM>(p[e], a.gamma, l1, d1);
                l[e] = (1.0f - k) * l[e] + k * a.a1 * l1;
                d[e] = (1.0f - k) * d[e] + k * a.a1 * d1;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < N; ++e) {
        acc += w[e] * l[e];
        d[e] *= gs * w[e];
    }
}

// U lane vectors in flight per wave and body step: 4 KB of logits per wave (4 fp32 / 2 bf16 vectors per lane).
template <typename T, int GM>
__global__ void __launch_bounds__(256) sigmoid_focal_kernel(Args a) {
    constexpr int V = VT<T>::V, U = sizeof(T) == 2 ? 2 : 4;
    extern __shared__ float w_lds[];
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const int nwaves = gridDim.x * wpb;
    int wsrc = a.w == nullptr ? 0 : 2;
    if (a.w != nullptr && a.C <= kLdsWeights) {               // block-uniform
        for (int i = threadIdx.x; i < a.C; i += blockDim.x) w_lds[i] = a.w[i];
        __syncthreads();
        wsrc = 1;
    }
    float wave_loss = 0.f;
    for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < a.B; row += nwaves) {
        const int r = __builtin_amdgcn_readfirstlane(row);
        const T* x = static_cast<const T*>(a.x) + (int64_t)r * a.ldx;
        T* dx = a.dx ? static_cast<T*>(a.dx) + (int64_t)r * a.lddx : nullptr;
        int64_t ta = a.ta[r];                                    // scalar loads: the row index is wave-uniform
        int64_t tb = a.tb ? a.tb[r] : -1;
        const bool bad = ta < 0 || ta >= a.C || (a.tb && (tb < 0 || tb >= a.C));
        if (bad && a.status && lane == 0) atomicExch(a.status, 1);
        if (bad) { ta = -1; tb = -1; }
        const float gs = bad ? 0.0f : a.scale;                   // a row with an out-of-range target contributes zero
        // head: elements before the first 16-byte boundary; body: nb lane vectors; rest: tail (one element per lane)
        int h = a.C, nb = 0;
        if (a.vec) {
            const int ph = (int)((reinterpret_cast<uintptr_t>(x) & 15u) / sizeof(T));
            h = ph ? V - ph : 0;
            if (h > a.C) h = a.C;
            nb = (a.C - h) / V;
        }
        float acc = 0.f;
        for (int v0 = 0; v0 < nb; v0 += 64 * U) {
            typename VT<T>::Raw raw[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const int v = v0 + j * 64 + lane;
                if (v < nb) raw[j] = VT<T>::raw(x + h + v * V);
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const int v = v0 + j * 64 + lane;
                if (v < nb) {
                    float xv[V], d[V];
                    VT<T>::unpack(raw[j], xv);
                    columns<GM, V>(a, wsrc, w_lds, xv, h + v * V, (int)ta, (int)tb, gs, acc, d);
                    if (dx) VT<T>::store(dx + h + v * V, d);
                }
            }
        }
        const int ns = a.C - nb * V;                              // head + tail elements
        for (int k = lane; k < ns; k += 64) {
            const int c = k < h ? k : k + nb * V;
            float xv[1] = {VT<T>::load1(x + c)}, d[1];
            columns<GM, 1>(a, wsrc, w_lds, xv, c, (int)ta, (int)tb, gs, acc, d);
            if (dx) VT<T>::store1(dx + c, d[0]);
        }
        acc = bad ? 0.0f : wave_sum(acc);
        if (lane == 0) a.loss_row[r] = acc;
        wave_loss += acc;
    }
    if (a.ticket != nullptr) ticketed_finish<1>(a.ticket, {wave_loss}, {a.scale}, {a.loss_out});       // loss_reduce.h
}

template <typename T>
int launch(const Args& a, int gm, hipStream_t st) {
    const int wpb = 4;
    const unsigned want = (unsigned)((a.B + wpb - 1) / wpb);
    const dim3 grid(want < kCePartialSlots ? want : kCePartialSlots), block(64 * wpb);
    const size_t lds = (a.w != nullptr && a.C <= kLdsWeights) ? (size_t)a.C * sizeof(float) : 0;
    switch (gm) {
        case 0: hipLaunchKernelGGL((sigmoid_focal_kernel<T, 0>), grid, block, lds, st, a); break;
        case 1: hipLaunchKernelGGL((sigmoid_focal_kernel<T, 1>), grid, block, lds, st, a); break;
        case 2: hipLaunchKernelGGL((sigmoid_focal_kernel<T, 2>), grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL((sigmoid_focal_kernel<T, 3>), grid, block, lds, st, a); break;
    }
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // namespace

extern "C" {

int iif_sigmoid_focal_fwd_bwd(const void* logits, int dtype, int64_t ld_logits, const int64_t* targets_a,
                              const int64_t* targets_b, float lam, const float* class_weight, float gamma,
                              int use_alpha, float alpha, float scale, int B, int C, float* loss_per_row,
                              float* loss_out, void* dlogits, int64_t ld_dlogits, int32_t* d_status,
                              void* d_workspace, void* stream) {
    if (B < 0 || C <= 0) return IIF_EINVAL;
    if (dtype != IIF_F32 && dtype != IIF_BF16) return IIF_EINVAL;
    if (!(gamma >= 0.0f) || gamma > 1e30f) return IIF_EINVAL;          // NaN, negative or infinite
    hipStream_t st = as_stream(stream);
    if (B == 0) {
        if (loss_out) {
            if (hipMemsetAsync(loss_out, 0, sizeof(float), st) != hipSuccess) return IIF_ELAUNCH;
        }
        return IIF_OK;
    }
    if (!logits || !targets_a || !loss_per_row) return IIF_EINVAL;
    if (ld_logits < C || (dlogits && ld_dlogits < C)) return IIF_EINVAL;
    const size_t es = dtype == IIF_F32 ? 4 : 2;
    const uintptr_t xp = reinterpret_cast<uintptr_t>(logits), dp = reinterpret_cast<uintptr_t>(dlogits);
    if (xp % es != 0 || dp % es != 0) return IIF_EINVAL;
    // the 16-byte body needs dlogits rows in the logits rows' 16-byte phase
    const bool vec = dlogits == nullptr || ((xp - dp) % 16 == 0 && ((uint64_t)(ld_logits - ld_dlogits) * es) % 16 == 0);
    const bool one_launch = loss_out != nullptr && d_workspace != nullptr;
    const bool focal = gamma > 0.0f;
    const bool alpha_on = focal && use_alpha;                 // custom.py:65-72: alpha only on the gamma > 0 branch
    Args a{};
    a.x = logits; a.ldx = ld_logits;
    a.ta = targets_a; a.tb = targets_b;
    a.la = targets_b ? lam : 1.0f; a.lb = targets_b ? 1.0f - lam : 0.0f;
    a.w = class_weight;
    a.gamma = gamma;
    a.a0 = alpha_on ? 1.0f - alpha : 1.0f;
    a.a1 = alpha_on ? alpha : 1.0f;
    a.scale = scale;
    a.B = B; a.C = C;
    a.loss_row = loss_per_row;
    a.dx = dlogits; a.lddx = ld_dlogits;
    a.status = d_status;
    a.loss_out = one_launch ? loss_out : nullptr;
    a.ticket = one_launch ? static_cast<int32_t*>(d_workspace) : nullptr;
    a.vec = vec ? 1 : 0;
    const int gm = !focal ? 0 : (gamma == 1.0f ? 1 : (gamma == 2.0f ? 2 : 3));
    const int rc = dtype == IIF_F32 ? launch<float>(a, gm, st) : launch<unsigned short>(a, gm, st);
    if (rc != IIF_OK) return rc;
    if (loss_out && !one_launch) {
        hipLaunchKernelGGL(rows_reduce_kernel<float>, dim3(1), dim3(256), 0, st, loss_per_row, B, scale, loss_out);
        IIF_LAUNCH_CHECK();
    }
    return IIF_OK;
}

}  // extern "C"
