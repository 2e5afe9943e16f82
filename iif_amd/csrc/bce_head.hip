// Detection-style sigmoid BCE head for gfx950 (MI355X): mmdet's binary_cross_entropy.
//
// instance_segmentation/mmdet/models/losses/cross_entropy_loss.py:53-111 + losses/utils.py:29-55 expand the labels to
// a one-hot [N, C] matrix and a [N, C] weight matrix on the device, run binary_cross_entropy_with_logits, multiply and
// reduce: ~10 launches and four [N, C] temporaries plus autograd.  Here ONE launch reads the logits once and writes
// d(loss)/d(logits), optionally the [N, C] element losses, and the scalar loss.
//
// The two real shapes sit at opposite ends: [1024 .. 8192, 1203 .. 1205] (the LVIS classifier) and [~500 000, 1] (RPN
// objectness).  A wave per row starves on the second, a register-resident row caps C.  So the kernel walks the FLAT
// element range e = i C + c of a contiguous [N, C] tensor in 16-byte lane vectors (4 fp32 / 8 bf16 elements) and
// carries the (row, column) of each vector along: one division per thread at the start, then (i, c) += the grid
// stride's (quotient, remainder) by C.  Inside a vector the column counts up and wraps into the next row, whose label
// and weight are then fetched: any C >= 1 works, C = 1 is simply "every element wraps".  The label and the row weight
// are read once per vector (all lanes of a wave read the same few rows when C is large: one cache line).
//   * C not a multiple of 4 / 8: vectors straddle rows; handled by the wrap above, no per-row head / tail.
//   * base not on a 16-byte boundary: the first h < V elements up to the boundary and the < V after the last whole
//     vector are done one per lane by the last block.  Every other array must put element h on a 16-byte boundary too
//     (dpred and loss_elems allocated by the caller with the logits' phase do); otherwise:
//   * a row pitch other than C, or an array out of phase: the same kernel body at V = 1, one element per lane
//     (coalesced dword / word accesses, addresses i ld + c).  Correct for every layout, not the fast path.
// Indexing is 64-bit throughout; there is no upper limit on C.
//
// Per element (x = logit; sp = softplus, s = sigmoid(x), q = 1 - s from the stable element of head_math.h):
//   labels:  y = 0: l = sp(x),  dl/dx = s          y = 1: l = pw_c sp(-x),  dl/dx = -pw_c q
//   dense :  l = (1 - y) sp(x) + pw_c y sp(-x),   dl/dx = (1 - y) s - pw_c y q
// which is torch's (1 - y) x + (1 + (pw - 1) y) sp(-x) with x + sp(-x) written as sp(x): exact at every |x|.
// The scalar loss leaves the same launch by the ticketed reduction of loss_reduce.h: no float atomics, bit-identical from
// call to call.
#include "common.h"
#include "head_math.h"
#include "loss_reduce.h"
#include "vec16.h"

namespace {

constexpr int kThreads = 256;

struct Args {
    const void* x; int64_t ldx;
    void* dx; int64_t lddx;
    const int64_t* labels; const float* rw; int64_t ignore;     // label mode
    const float* tgt; const float* ew;                          // dense mode ([N, C] contiguous)
    const float* cw;                                            // pos_weight [C] or nullptr
    float scale;
    int N, C;
    float* elems;                 // [N, C] contiguous or nullptr
    float* loss_out; int32_t* ticket;
    int h;                        // elements before the first whole vector (V > 1)
    int64_t nv;                   // whole vectors (V = 1: elements)
    unsigned qs, rs;              // grid stride in elements = qs * C + rs
};

// weight (0 for an ignored row) and target column (-1: none, a background row) of row i
__device__ __forceinline__ void load_row(const Args& a, int64_t i, float& wi, int& t) {
    const int64_t lab = a.labels[i];
    const float w = a.rw ? a.rw[i] : 1.0f;          // not under `valid`: the two loads are in flight together
    const bool valid = lab >= 0 && lab != a.ignore;
    wi = valid ? w : 0.0f;
    t = (valid && lab < (int64_t)a.C) ? (int)lab : -1;
}

// unscaled weighted loss l and d l / d x of one element.  DENSE: y / ew are its target and weight; else wi / t its row's.
template <bool DENSE>
__device__ __forceinline__ void one(const Args& a, float x, int c, float wi, int t, float y, float ew, float& l, float& d) {
    if constexpr (DENSE) {
        const SigmoidElem p = sigmoid_elem(x);
        const float pw = a.cw ? a.cw[c] : 1.0f;
        l = ((1.0f - y) * p.spp + pw * y * p.spn) * ew;
        d = ((1.0f - y) * p.s - pw * y * p.q) * ew;
    } else {
        bce_label_elem(x, c, t, wi, a.cw, l, d);             // head_math.h
    }
}

template <int V> constexpr int unroll_of() { return V == 8 ? 2 : 4; }       // vectors in flight per lane and step (fp32: 64 bytes)
constexpr int kSmallGrid = 256;                // one step of work is spread over at most this many blocks (one per CU)

// V > 1: pred / dpred are contiguous (e = i C + c is the address) and every array has element a.h on a 16-byte boundary.
// V = 1: any pitch, any element-aligned base.
template <typename T, bool DENSE, int V>
__global__ void __launch_bounds__(kThreads) bce_det_kernel(Args a) {
    constexpr int U = unroll_of<V>();
    const T* x = static_cast<const T*>(a.x);
    T* dx = static_cast<T*>(a.dx);
    const int64_t T_ = (int64_t)gridDim.x * kThreads;                      // vectors per grid step
    const int64_t gtid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const unsigned C = (unsigned)a.C;
    // (row, column) of this thread's first vector; its flat index is below 2^32 (at most kCePartialSlots * 256 * 8 + 7)
    const unsigned e_first = (unsigned)a.h + (unsigned)gtid * V;
    int64_t i = e_first / C;
    unsigned c = e_first % C;
    float acc = 0.f;
    for (int64_t v0 = gtid; v0 < a.nv; v0 += U * T_) {
        int64_t iv[U];
        unsigned cv[U];
        typename VTn<T, V>::Raw raw[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            iv[j] = i; cv[j] = c;
            i += a.qs; c += a.rs;
            if (c >= C) { c -= C; ++i; }
            const int64_t v = v0 + j * T_;
            if (v < a.nv) raw[j] = VTn<T, V>::raw(V == 1 ? x + iv[j] * a.ldx + cv[j] : x + a.h + v * V);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int64_t v = v0 + j * T_;
            if (v >= a.nv) continue;
            const int64_t e = V == 1 ? v : a.h + v * V;                    // flat logical index of the first element
            float xv[V], lv[V], dv[V], yv[V], wv[V];
            VTn<T, V>::unpack(raw[j], xv);
            int64_t ii = iv[j];
            int ci = (int)cv[j];
            float wi = 1.0f;
            int t = -1;
            if constexpr (DENSE) {
                load_f32<V>(a.tgt + e, yv);
                if (a.ew) load_f32<V>(a.ew + e, wv);
            } else {
                load_row(a, ii, wi, t);
            }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                one<DENSE>(a, xv[k], ci, wi, t, DENSE ? yv[k] : 0.0f, (DENSE && a.ew) ? wv[k] : 1.0f, lv[k], dv[k]);
                acc += lv[k];
                dv[k] *= a.scale;
                if (k + 1 < V && ++ci == a.C) {                            // the vector runs on into the next row
                    ci = 0;
                    ++ii;
                    if constexpr (!DENSE) {
                        if (ii < (int64_t)a.N) load_row(a, ii, wi, t);
                    }
                }
            }
            if (dx) VTn<T, V>::store(V == 1 ? dx + iv[j] * a.lddx + cv[j] : dx + e, dv);
            if (a.elems) store_f32<V>(a.elems + e, lv);
        }
    }
    if constexpr (V > 1) {
        // the elements in front of the first and behind the last whole vector (fewer than 2 V), one per lane of the last block
        const int64_t M = (int64_t)a.N * a.C;
        const int64_t body_end = a.h + a.nv * V;
        const int ne = a.h + (int)(M - body_end);
        if (blockIdx.x == gridDim.x - 1 && (int)threadIdx.x < ne) {
            const int64_t e = (int)threadIdx.x < a.h ? (int64_t)threadIdx.x : body_end + ((int)threadIdx.x - a.h);
            const int64_t ii = e / a.C;
            const int ci = (int)(e - ii * a.C);
            float wi = 1.0f, l, d;
            int t = -1;
            if constexpr (!DENSE) load_row(a, ii, wi, t);
            float xv[1];
            VTn<T, 1>::load(x + e, xv);
            one<DENSE>(a, xv[0], ci, wi, t, DENSE ? a.tgt[e] : 0.0f, (DENSE && a.ew) ? a.ew[e] : 1.0f, l, d);
            acc += l;
            if (dx) { const float dd[1] = {d * a.scale}; VTn<T, 1>::store(dx + e, dd); }
            if (a.elems) a.elems[e] = l;
        }
    }
    if (a.ticket != nullptr) ticketed_finish<1>(a.ticket, {wave_sum(acc)}, {a.scale}, {a.loss_out});       // loss_reduce.h
}

template <typename T, bool DENSE, int V>
int launch(Args a, hipStream_t st) {
    // Every block publishes a partial and takes a ticket on one address, so a small problem wants few blocks: up to kSmallGrid
    // blocks whose threads take k <= U vectors in their one step; beyond that whole steps of U vectors per thread, the same
    // number of steps in every block.
    constexpr int U = unroll_of<V>();
    const int64_t blocks1 = a.nv > 0 ? cdiv64(a.nv, kThreads) : 1;          // at one vector per thread
    const int64_t k = cdiv64(blocks1, kSmallGrid);
    unsigned grid;
    if (k <= U) {
        grid = (unsigned)cdiv64(blocks1, k);
    } else {
        const int64_t units = cdiv64(blocks1, U);
        const int64_t iters = cdiv64(units, kCePartialSlots);
        grid = (unsigned)cdiv64(units, iters);
    }
    const uint64_t stride = (uint64_t)grid * kThreads * V;                  // elements from one of a thread's vectors to the next
    a.qs = (unsigned)(stride / (uint64_t)a.C);
    a.rs = (unsigned)(stride % (uint64_t)a.C);
    hipLaunchKernelGGL((bce_det_kernel<T, DENSE, V>), dim3(grid), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

template <typename T, int V>
int launch_mode(const Args& a, hipStream_t st) {
    return a.tgt ? launch<T, true, V>(a, st) : launch<T, false, V>(a, st);
}

}  // namespace

extern "C" {

int iif_bce_det_fwd_bwd(const void* pred, int dtype, int64_t ld_pred, const int64_t* labels, const float* row_weight,
                        int64_t ignore_index, const float* targets, const float* elem_weight, const float* class_weight,
                        float scale, int N, int C, float* loss_elems, float* loss_out, void* dpred, int64_t ld_dpred,
                        void* d_workspace, void* stream) {
    if (N < 0 || C <= 0) return IIF_EINVAL;
    if (dtype != IIF_F32 && dtype != IIF_BF16) return IIF_EINVAL;
    hipStream_t st = as_stream(stream);
    if (N == 0) {                                                           // (an empty tensor's pointers may all be null)
        if (loss_out) {
            if (hipMemsetAsync(loss_out, 0, sizeof(float), st) != hipSuccess) return IIF_ELAUNCH;
        }
        return IIF_OK;
    }
    if ((labels != nullptr) == (targets != nullptr)) return IIF_EINVAL;     // exactly one of the two modes
    if (labels && elem_weight) return IIF_EINVAL;
    if (targets && row_weight) return IIF_EINVAL;
    if (loss_out && !d_workspace) return IIF_EINVAL;
    if (!pred) return IIF_EINVAL;
    if (ld_pred < C || (dpred && ld_dpred < C)) return IIF_EINVAL;
    const size_t es = dtype == IIF_F32 ? 4 : 2;
    const uintptr_t xp = reinterpret_cast<uintptr_t>(pred), dp = reinterpret_cast<uintptr_t>(dpred);
    if (xp % es != 0 || dp % es != 0) return IIF_EINVAL;
    const uintptr_t f32s[] = {reinterpret_cast<uintptr_t>(loss_elems), reinterpret_cast<uintptr_t>(targets),
                              reinterpret_cast<uintptr_t>(elem_weight)};
    for (uintptr_t p : f32s)
        if (p % 4 != 0) return IIF_EINVAL;
    Args a{};
    a.x = pred; a.ldx = ld_pred;
    a.dx = dpred; a.lddx = ld_dpred;
    a.labels = labels; a.rw = row_weight; a.ignore = ignore_index;
    a.tgt = targets; a.ew = elem_weight;
    a.cw = class_weight;
    a.scale = scale;
    a.N = N; a.C = C;
    a.elems = loss_elems;
    a.loss_out = loss_out;
    a.ticket = loss_out ? static_cast<int32_t*>(d_workspace) : nullptr;
    const int64_t M = (int64_t)N * C;
    // the flat 16-byte form: contiguous rows, and element h (the first on a 16-byte boundary of pred) on a 16-byte boundary of
    // every other array
    const int V = (int)(16 / es);
    const int64_t h = (int64_t)(((16 - xp % 16) % 16) / es);
    bool flat = (N == 1 || ld_pred == C) && (!dpred || N == 1 || ld_dpred == C);
    flat = flat && (!dpred || (dp + h * es) % 16 == 0);
    for (uintptr_t p : f32s) flat = flat && (p == 0 || (p + h * 4) % 16 == 0);
    if (flat) {
        a.h = (int)(h < M ? h : M);
        a.nv = (M - a.h) / V;
        return dtype == IIF_F32 ? launch_mode<float, 4>(a, st) : launch_mode<unsigned short, 8>(a, st);
    }
    a.h = 0;
    a.nv = M;
    return dtype == IIF_F32 ? launch_mode<float, 1>(a, st) : launch_mode<unsigned short, 1>(a, st);
}

}  // extern "C"
