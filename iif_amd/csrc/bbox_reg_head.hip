// Box-regression loss head for gfx950 (MI355X): mmdet's l1_loss / smooth_l1_loss and the positive-row gather of BBoxHead.loss.
//
// instance_segmentation/mmdet/models/roi_heads/bbox_heads/bbox_head.py:284-311 forms pos_inds, asks pos_inds.any() (a host
// round trip), boolean-indexes bbox_pred.view(N, -1, 4)[pos_inds, labels[pos_inds]], bbox_targets and bbox_weights (three
// nonzero()s, three more round trips) and runs losses/smooth_l1_loss.py:10-52 + losses/utils.py:29-55 on the result; autograd
// then builds a zero [N, 4C] tensor and an index_put into it.  With the LVIS head that tensor is [1024, 4812] fp32, 19.7 MB,
// for a loss that reads 1024 x 16 bytes of it.  Here:
//
//   iif_bbox_reg_fwd           ONE launch: the scalar loss, the COMPACT gradient dsel [n] fp32 (n = 4N: one 16-byte row per
//                              box) and optionally the element losses.  Gather mode reads the row's label and, for a positive
//                              row, the four deltas of its class straight out of pred [N, 4C]; plain mode (the modules, RPN)
//                              walks a flat range.  The forward touches ~50 KB at the LVIS shape.
//   iif_bbox_reg_scatter_grad  ONE launch, a pure store stream: dpred [N, 4C] = g * dsel[i] at row i, columns 4 label_i .. +3
//                              of the positive rows and zero everywhere else, every byte written exactly once (no memset, no
//                              fill-then-overwrite).  g is the upstream gradient, a device scalar.
//
// The dense gradient is therefore written once, already scaled, in backward; producing it in forward (as bce_head.hip does,
// where every element carries a gradient) would cost the 19.7 MB write plus a 39 MB read-and-write for the upstream scaling.
//
// Forward, per lane: V = 4 consecutive elements = one box (16 bytes of fp32 target / weight / dsel; 16 bytes of fp32 or 8 of
// bf16 pred) when every array's phase allows it, else V = 1, one element per lane, any element-aligned base and pitch.
// Scatter, per lane: one 16-byte piece of dpred = one class slot (4 fp32 deltas) or two (2 x 4 bf16 deltas; with odd C a piece
// straddles two rows, so alternate rows sit on the other 8-byte phase and the slots of a piece are looked up separately).  The
// (row, class) of a lane's piece is carried along as in bce_head.hip: one division at the start, then += the grid stride's
// (quotient, remainder) by C.  A base off the 16-byte boundary or a pitch other than 4C runs one element per lane.
//
// Per element: d = p - t, a = |d|;  L1 (beta = 0): l = a, dl = sign(d) with sign(0) = 0 (torch's abs backward);
// smooth L1: a < beta ? (0.5 a a / beta, d / beta) : (a - 0.5 beta, sign(d)), the comparison strict as in the reference (so
// beta = 0 IS L1: no branch on the mode).  loss = scale * sum w l, dsel = scale * w * dl, loss_elems = w * l.
// The scalar leaves the forward launch by the ticketed reduction of loss_reduce.h: no float atomics, a fixed summation order,
// bit-identical from call to call.  Indexing is 64-bit.
#include "common.h"
#include "loss_reduce.h"
#include "vec16.h"

namespace {

constexpr unsigned kScatterBlocks = 2048;      // scatter grid cap (the scatter launches use no workspace)
constexpr int kThreads = 256;
constexpr unsigned kFwdBlocks = 1024;          // forward grid cap: 16 waves per CU, each with a box's three 16-byte loads in flight
static_assert(kFwdBlocks <= kCePartialSlots, "one partial slot per forward block");
constexpr int kSmallGrid = 256;                // scatter: one step of work is spread over at most this many blocks (one per CU)
constexpr int kU = 4;                          // scatter: 16-byte stores in flight per lane and step

struct FwdArgs {
    const void* pred; int64_t ld;
    const int64_t* labels; int64_t num_classes; int agnostic;       // gather mode (labels != nullptr)
    const float* tgt; const float* w;
    float beta, scale;
    int64_t n;
    float* dsel; float* elems;
    float* loss_out; int32_t* ticket;
};

struct ScatterArgs {
    const float* dsel; const int64_t* labels; int64_t num_classes; int agnostic;
    const float* g;
    void* d; int64_t ld;
    int N, C;
    int64_t nv;                   // whole 16-byte pieces (vector form)
    unsigned qs, rs;              // grid stride in class slots = qs * C + rs
};

// unscaled weighted loss l = w * loss(p, t) and the scaled gradient g = scale * w * d loss / d p of one element
__device__ __forceinline__ void one(const FwdArgs& a, float p, float t, float w, float& l, float& g) {
    const float d = p - t;
    const float ad = fabsf(d);
    const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    float dl;
    if (ad < a.beta) {
        l = 0.5f * ad * ad / a.beta;
        dl = d / a.beta;
    } else {
        l = ad - 0.5f * a.beta;
        dl = sg;
    }
    l *= w;
    g = a.scale * w * dl;
}

__device__ __forceinline__ bool positive(int64_t lab, int64_t num_classes) { return lab >= 0 && lab < num_classes; }

// The V elements from flat index e on (V = 4: e is a multiple of 4, one box).  Returns the sum of their weighted losses.
template <typename T, int V>
__device__ __forceinline__ float unit(const FwdArgs& a, int64_t e) {
    const T* pred = static_cast<const T*>(a.pred);
    const T* src = pred + e;
    bool pos = true;
    if (a.labels) {
        const int64_t row = e >> 2;
        const int64_t lab = a.labels[row];
        pos = positive(lab, a.num_classes);
        src = pred + row * a.ld + (a.agnostic ? 0 : 4 * lab) + (e & 3);      // dereferenced for a positive row only
    }
    float p[V], t[V], w[V], l[V], g[V];
    load_f32<V>(a.tgt + e, t);
    if (a.w) load_f32<V>(a.w + e, w);
    if (pos) VTn<T, V>::load(src, p);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        l[k] = 0.0f; g[k] = 0.0f;
        if (pos) one(a, p[k], t[k], a.w ? w[k] : 1.0f, l[k], g[k]);
        acc += l[k];
    }
    if (a.dsel) store_f32<V>(a.dsel + e, g);
    if (a.elems) store_f32<V>(a.elems + e, l);
    return acc;
}

// V = 4: pred's boxes on a 4-element boundary of T (16 bytes fp32, 8 bytes bf16), every fp32 array on a 16-byte boundary;
// the n % 4 elements behind the last whole box (plain mode only) go one per lane.  V = 1: anything element-aligned.
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) bbox_reg_fwd_kernel(FwdArgs a) {
    const int64_t T_ = (int64_t)gridDim.x * kThreads;
    const int64_t gtid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nu = a.n / V;
    float acc = 0.f;
    for (int64_t u = gtid; u < nu; u += T_) acc += unit<T, V>(a, u * V);
    if constexpr (V > 1) {
        const int64_t e = nu * V + threadIdx.x;
        if (blockIdx.x == gridDim.x - 1 && e < a.n) acc += unit<T, 1>(a, e);
    }
    if (a.ticket != nullptr) ticketed_finish<1>(a.ticket, {wave_sum(acc)}, {a.scale}, {a.loss_out});       // loss_reduce.h
}

template <typename T, int V>
int launch_fwd(const FwdArgs& a, hipStream_t st) {
    int64_t blocks = cdiv64(a.n / V, kThreads);
    blocks = blocks < 1 ? 1 : (blocks > kFwdBlocks ? kFwdBlocks : blocks);
    hipLaunchKernelGGL((bbox_reg_fwd_kernel<T, V>), dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

// g * dsel[i, 0..3] if (i, c) is the class slot of a positive row i, else zeros
__device__ __forceinline__ f32x4 slot_value(const ScatterArgs& a, int64_t i, unsigned c, int64_t lab, float g) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (positive(lab, a.num_classes) && (a.agnostic ? 0 : lab) == (int64_t)c) {
        const float* s = a.dsel + 4 * i;
        v = f32x4{g * s[0], g * s[1], g * s[2], g * s[3]};
    }
    return v;
}

// dpred contiguous ([N, 4C], pitch 4C) on a 16-byte boundary.  S = class slots per 16-byte piece: 1 (fp32) or 2 (bf16).
template <typename T, int S>
__global__ void __launch_bounds__(kThreads) bbox_reg_scatter_vec_kernel(ScatterArgs a) {
    T* d = static_cast<T*>(a.d);
    const float g = a.g ? *a.g : 1.0f;
    const int64_t T_ = (int64_t)gridDim.x * kThreads;                      // pieces per grid step
    const int64_t gtid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const unsigned C = (unsigned)a.C;
    // (row, class) of the first slot of this thread's first piece; the slot index is below 2^32 (at most 2048 * 256 * 2 + 1)
    const unsigned s_first = (unsigned)gtid * S;
    int64_t i = s_first / C;
    unsigned c = s_first % C;
    for (int64_t v0 = gtid; v0 < a.nv; v0 += kU * T_) {
        int64_t iv[kU][S], lab[kU][S];
        unsigned cv[kU][S];
#pragma unroll
        for (int j = 0; j < kU; ++j) {
            iv[j][0] = i; cv[j][0] = c;
            if constexpr (S == 2) {
                const bool wrap = c + 1 == C;
                iv[j][1] = wrap ? i + 1 : i;
                cv[j][1] = wrap ? 0u : c + 1;
            }
            i += a.qs; c += a.rs;
            if (c >= C) { c -= C; ++i; }
            if (v0 + j * T_ < a.nv) {                                      // (both slots of a whole piece are inside [N, C])
#pragma unroll
                for (int s = 0; s < S; ++s) lab[j][s] = a.labels[iv[j][s]];
            }
        }
#pragma unroll
        for (int j = 0; j < kU; ++j) {
            const int64_t v = v0 + j * T_;
            if (v >= a.nv) continue;
            if constexpr (S == 1) {
                *reinterpret_cast<f32x4*>(d + v * 4) = slot_value(a, iv[j][0], cv[j][0], lab[j][0], g);
            } else {
                const f32x4 lo = slot_value(a, iv[j][0], cv[j][0], lab[j][0], g), hi = slot_value(a, iv[j][1], cv[j][1], lab[j][1], g);
                // (packed before the address is formed: the two orders schedule differently)
                *reinterpret_cast<u32x4*>(d + v * 8) = VT<T>::pack({lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w});
            }
        }
    }
    if constexpr (S == 2) {
        // N C odd: the last class slot is half a piece, 8 bytes, written by one lane
        const int64_t slots = (int64_t)a.N * a.C;
        if ((slots & 1) && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
            const int64_t il = a.N - 1;
            const f32x4 v = slot_value(a, il, C - 1, a.labels[il], g);
            *reinterpret_cast<u32x2*>(d + (slots - 1) * 4) = VT<T>::pack4({v.x, v.y, v.z, v.w});
        }
    }
}

// any element-aligned base, any pitch >= 4C: one element per lane, the columns [0, 4C) of every row
template <typename T>
__global__ void __launch_bounds__(kThreads) bbox_reg_scatter_elem_kernel(ScatterArgs a) {
    T* d = static_cast<T*>(a.d);
    const float g = a.g ? *a.g : 1.0f;
    const int64_t T_ = (int64_t)gridDim.x * kThreads;
    const int64_t W = 4 * (int64_t)a.C;
    const int64_t M = (int64_t)a.N * W;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < M; e += T_) {
        const int64_t i = e / W;
        const int64_t col = e - i * W;
        const int64_t lab = a.labels[i];
        float v = 0.0f;
        if (positive(lab, a.num_classes) && (a.agnostic ? 0 : lab) == (col >> 2)) v = g * a.dsel[4 * i + (col & 3)];
        VT<T>::store1(d + i * a.ld + col, v);
    }
}

template <typename T, int S>
int launch_scatter_vec(ScatterArgs a, hipStream_t st) {
    // as bce_head.hip: up to kSmallGrid blocks whose threads take k <= kU pieces in their one step; beyond that whole steps of kU
    // pieces per thread, the same number of steps in every block
    const int64_t blocks1 = a.nv > 0 ? cdiv64(a.nv, kThreads) : 1;
    const int64_t k = cdiv64(blocks1, kSmallGrid);
    unsigned grid;
    if (k <= kU) {
        grid = (unsigned)cdiv64(blocks1, k);
    } else {
        const int64_t units = cdiv64(blocks1, kU);
        const int64_t iters = cdiv64(units, kScatterBlocks);
        grid = (unsigned)cdiv64(units, iters);
    }
    const uint64_t stride = (uint64_t)grid * kThreads * S;                  // class slots from one of a thread's pieces to the next
    a.qs = (unsigned)(stride / (uint64_t)a.C);
    a.rs = (unsigned)(stride % (uint64_t)a.C);
    hipLaunchKernelGGL((bbox_reg_scatter_vec_kernel<T, S>), dim3(grid), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

template <typename T>
int launch_scatter_elem(const ScatterArgs& a, hipStream_t st) {
    int64_t blocks = cdiv64((int64_t)a.N * 4 * a.C, kThreads);
    blocks = blocks > kScatterBlocks ? kScatterBlocks : blocks;
    hipLaunchKernelGGL((bbox_reg_scatter_elem_kernel<T>), dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // namespace

extern "C" {

int iif_bbox_reg_fwd(const void* pred, int dtype, int64_t ld_pred, const int64_t* labels, int num_classes, int C,
                     const float* target, const float* weight, float beta, float scale, int64_t n, int N,
                     float* loss_elems, float* loss_out, float* dsel, void* d_workspace, void* stream) {
    if (n < 0 || N < 0 || C <= 0) return IIF_EINVAL;
    if (dtype != IIF_F32 && dtype != IIF_BF16) return IIF_EINVAL;
    if (!(beta >= 0.0f)) return IIF_EINVAL;
    hipStream_t st = as_stream(stream);
    if (n == 0) {                                                           // (an empty tensor's pointers may all be null)
        if (loss_out) {
            if (hipMemsetAsync(loss_out, 0, sizeof(float), st) != hipSuccess) return IIF_ELAUNCH;
        }
        return IIF_OK;
    }
    if (labels) {
        if (n != 4 * (int64_t)N || num_classes < 1 || ld_pred < 4 * (int64_t)C) return IIF_EINVAL;
        if (C > 1 && num_classes > C) return IIF_EINVAL;                    // a positive label indexes pred's classes
    } else if (C != 1) {
        return IIF_EINVAL;
    }
    if (!pred || !target) return IIF_EINVAL;
    if (loss_out && !d_workspace) return IIF_EINVAL;
    const size_t es = dtype == IIF_F32 ? 4 : 2;
    const uintptr_t xp = reinterpret_cast<uintptr_t>(pred);
    if (xp % es != 0) return IIF_EINVAL;
    const uintptr_t f32s[] = {reinterpret_cast<uintptr_t>(target), reinterpret_cast<uintptr_t>(weight),
                              reinterpret_cast<uintptr_t>(loss_elems), reinterpret_cast<uintptr_t>(dsel)};
    for (uintptr_t p : f32s)
        if (p % 4 != 0) return IIF_EINVAL;
    FwdArgs a{};
    a.pred = pred; a.ld = ld_pred;
    a.labels = labels; a.num_classes = num_classes; a.agnostic = C == 1;
    a.tgt = target; a.w = weight;
    a.beta = beta; a.scale = scale;
    a.n = n;
    a.dsel = dsel; a.elems = loss_elems;
    a.loss_out = loss_out;
    a.ticket = loss_out ? static_cast<int32_t*>(d_workspace) : nullptr;
    // a box per lane: pred's boxes on a 4-element boundary, the fp32 arrays on a 16-byte one
    bool vec = xp % (4 * es) == 0 && (!labels || ld_pred % 4 == 0);
    for (uintptr_t p : f32s) vec = vec && p % 16 == 0;
    if (vec) return dtype == IIF_F32 ? launch_fwd<float, 4>(a, st) : launch_fwd<unsigned short, 4>(a, st);
    return dtype == IIF_F32 ? launch_fwd<float, 1>(a, st) : launch_fwd<unsigned short, 1>(a, st);
}

int iif_bbox_reg_scatter_grad(const float* dsel, const int64_t* labels, int num_classes, int N, int C, const float* g,
                              void* dpred, int dtype, int64_t ld_dpred, void* stream) {
    if (N < 0 || C <= 0 || num_classes < 1) return IIF_EINVAL;
    if (dtype != IIF_F32 && dtype != IIF_BF16) return IIF_EINVAL;
    if (N == 0) return IIF_OK;
    if (C > 1 && num_classes > C) return IIF_EINVAL;
    if (!dsel || !labels || !dpred || ld_dpred < 4 * (int64_t)C) return IIF_EINVAL;
    const size_t es = dtype == IIF_F32 ? 4 : 2;
    const uintptr_t dp = reinterpret_cast<uintptr_t>(dpred);
    if (dp % es != 0 || reinterpret_cast<uintptr_t>(dsel) % 4 != 0) return IIF_EINVAL;
    hipStream_t st = as_stream(stream);
    ScatterArgs a{};
    a.dsel = dsel; a.labels = labels; a.num_classes = num_classes; a.agnostic = C == 1;
    a.g = g;
    a.d = dpred; a.ld = ld_dpred;
    a.N = N; a.C = C;
    if (dp % 16 == 0 && (N == 1 || ld_dpred == 4 * (int64_t)C)) {
        const int64_t slots = (int64_t)N * C;
        if (dtype == IIF_F32) {
            a.nv = slots;
            return launch_scatter_vec<float, 1>(a, st);
        }
        a.nv = slots / 2;
        return launch_scatter_vec<unsigned short, 2>(a, st);
    }
    return dtype == IIF_F32 ? launch_scatter_elem<float>(a, st) : launch_scatter_elem<unsigned short>(a, st);
}

}  // extern "C"
