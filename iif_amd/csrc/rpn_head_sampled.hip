// The RPN head's backward at the sampled pixels only, gfx950.
//
// Reference: RPNHead.forward_single (dense_heads/rpn_head.py:38-44) is h = relu(rpn_conv(x)) followed by the two 1x1 convolutions
// rpn_cls(h) and rpn_reg(h).  AnchorHead.loss_single weights every unsampled anchor by 0 and nothing else consumes the maps with
// a gradient, so the gradient that reaches the maps is zero outside the pixels of the sampled anchors: at most B (nep + num)
// pixels.  The forward stays on the modules' own convolutions; the backward never forms a dense tensor:
//   pixels    iif_rpn_sampled_pixels: slot e of the B (nep + num) entries -> (image, level, y, x).  Two sampled anchors of one pixel
//             make ONE active slot: an integer atomicMin into a cleared per-pixel owner map, the lowest slot index owns the pixel.
//   prepare   patchT [9 Ci + 1][S]: column s the 3x3 x Ci patch of slot s gathered through the tensor's strides (k = 9 ci + tap,
//             the weight's own order; taps outside the map and inactive slots are zeros), row 9 Ci all ones; g [S][5 A]: the
//             output gradients of the slot's pixel (zeros for an inactive slot); [W_cls; W_reg] stacked.
//   hidden    pre = patch . W_conv^T + b, h = relu(pre) (with a column of ones behind it), dh = (g . [W_cls; W_reg]) [pre > 0].
//   params    [dW_cls; dW_reg | db] = g^T [h | 1] and [dW_conv | db_conv] = dh^T [patch | 1]: the slots in split ranges, one
//             partial per range, the partials summed in range order.
//   input     T = dh . W_conv [S][9 Ci]; every affected pixel q is written ONCE as the sum over its at most nine contributing
//             slots in tap order.  The contributors of q are found through the owner map; of the candidates (slot, tap) that
//             reach q the one with the lowest slot index writes.  Everything else in d feats is the caller's clear.
// All products run on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: exact float32 products, a fixed-order chain per output), one
// wave per 32 x 32 tile, operands straight from global memory: an operand whose rows run along k is read four consecutive k at
// a time (lane half hf takes k0 + 4 hf .. + 3 of every eight), the other kind one coalesced row per k.  No float atomics, no
// data-dependent launch: the worst-case slot count sizes every grid; the same bits from call to call.
#include "common.h"
#include "rpn_grid.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int kThreads = 256;
constexpr int kMaxChannels = 2048;              // Ci, Co: multiples of 8
constexpr int kMaxSplits = 16, kMinPer = 64;    // slot ranges of the parameter pass
constexpr unsigned kNoOwner = 0xffffffffu;

__device__ __forceinline__ int crow(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }   // C/D row of register r

// acc[r] += sum_{k in [k0, k1)} A(row, k) B(k, col): row on the registers (crow), col on the lane.  KA: A(row, k) = a[row lda + k],
// else a[k lda + row]; KB: B(k, col) = b[col ldb + k], else b[k ldb + col].  `a` / `b` arrive offset to the lane's row / column;
// a lane whose row (column) is outside the matrix passes ok = false and contributes zeros.  k0, k1 multiples of 8.
template <bool KA, bool KB>
__device__ __forceinline__ void tile_mac(const float* __restrict__ a, int64_t lda, bool aok, const float* __restrict__ b, int64_t ldb,
                                         bool bok, int k0, int k1, int half, f32x16& acc) {
    for (int k = k0 + 4 * half; k < k1; k += 8) {
        f32x4 av = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
        if (aok) {
            if (KA) av = *reinterpret_cast<const f32x4*>(a + k);
            else { av.x = a[k * lda]; av.y = a[(k + 1) * lda]; av.z = a[(k + 2) * lda]; av.w = a[(k + 3) * lda]; }
        }
        if (bok) {
            if (KB) bv = *reinterpret_cast<const f32x4*>(b + k);
            else { bv.x = b[k * ldb]; bv.y = b[(k + 1) * ldb]; bv.z = b[(k + 2) * ldb]; bv.w = b[(k + 3) * ldb]; }
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------------ the sampled pixels
struct PixArgs { Grid g; Lists s; int pix_start[kMaxLevels]; int P; unsigned* owner; int* slots; };

__device__ __forceinline__ bool slot_pixel(const PixArgs& a, int e, int& b, Cell& c) {
    int slot;
    bool pos;
    const int64_t idx = entry_of(a.s, e, b, pos, slot);
    if (idx < 0 || idx >= a.g.A) return false;
    c = locate(a.g, (int)idx);
    return true;
}

__global__ void __launch_bounds__(kThreads) pixels_mark_kernel(PixArgs a) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= a.s.B * (a.s.nep + a.s.num)) return;
    int b;
    Cell c;
    if (!slot_pixel(a, e, b, c)) return;
    atomicMin(a.owner + (int64_t)b * a.P + a.pix_start[c.l] + c.y * a.g.lv[c.l].W + c.x, (unsigned)e);
}

__global__ void __launch_bounds__(kThreads) pixels_slots_kernel(PixArgs a) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= a.s.B * (a.s.nep + a.s.num)) return;
    int b = 0;
    Cell c;
    int l = -1, y = 0, x = 0;
    if (slot_pixel(a, e, b, c) && a.owner[(int64_t)b * a.P + a.pix_start[c.l] + c.y * a.g.lv[c.l].W + c.x] == (unsigned)e) {
        l = c.l; y = c.y; x = c.x;
    }
    int* o = a.slots + 4 * (int64_t)e;
    o[0] = l < 0 ? 0 : b; o[1] = l; o[2] = y; o[3] = x;
}

// ------------------------------------------------------------------------------------------------ the backward
struct HeadLvl {
    const float* feat; float* g_feat; const float* g_scores; const float* g_deltas;
    int64_t fs[4], gfs[4], gss[4], gds[4];
    int H, W, pix_start;
};

struct HeadArgs {
    HeadLvl lv[kMaxLevels];
    int L, P, S, SP, A, J, JP, ci, co, K;          // S slots, SP = S rounded up to 32; J = 5 A, JP = J rounded up to 8; K = 9 ci
    const unsigned* owner; const int* slots;
    const float* w_conv; const float* b_conv; const float* w_cls; const float* w_reg;
    float* patchT; float* g; float* wcr; float* h; float* dh; float* T;   // [K + 1][SP], [SP][JP], [JP][co], [SP][co + 1], [SP][co], [SP][K]
};

// patchT: block (64 slots, 64 values of k); lane = slot, the four waves take k in turn
__global__ void __launch_bounds__(kThreads) head_patch_kernel(HeadArgs a) {
    const int s = blockIdx.x * 64 + (threadIdx.x & 63);
    if (s >= a.SP) return;
    int b = 0, l = -1, y = 0, x = 0;
    if (s < a.S) { const int* o = a.slots + 4 * (int64_t)s; b = o[0]; l = o[1]; y = o[2]; x = o[3]; }
    const int kend = min((int)(blockIdx.y + 1) * 64, a.K + 1);
    for (int k = blockIdx.y * 64 + (threadIdx.x >> 6); k < kend; k += 4) {
        float v = 0.f;
        if (k == a.K) {
            v = 1.f;
        } else if (l >= 0) {
            const HeadLvl& lv = a.lv[l];
            const int c = k / 9, tap = k - 9 * c, yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            if (yy >= 0 && yy < lv.H && xx >= 0 && xx < lv.W) v = lv.feat[b * lv.fs[0] + c * lv.fs[1] + yy * lv.fs[2] + xx * lv.fs[3]];
        }
        a.patchT[(int64_t)k * a.SP + s] = v;
    }
}

// g [SP][JP], the ones behind h, and [W_cls; W_reg] with zero rows up to JP: one element per thread
__global__ void __launch_bounds__(kThreads) head_prep_kernel(HeadArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x, ng = (int64_t)a.SP * a.JP, nw = (int64_t)a.JP * a.co;
    if (i < ng) {
        const int s = (int)(i / a.JP), j = (int)(i - (int64_t)s * a.JP);
        float v = 0.f;
        if (s < a.S && j < a.J) {
            const int* o = a.slots + 4 * (int64_t)s;
            const int b = o[0], l = o[1], y = o[2], x = o[3];
            if (l >= 0) {
                const HeadLvl& lv = a.lv[l];
                v = j < a.A ? lv.g_scores[b * lv.gss[0] + j * lv.gss[1] + y * lv.gss[2] + x * lv.gss[3]]
                            : lv.g_deltas[b * lv.gds[0] + (j - a.A) * lv.gds[1] + y * lv.gds[2] + x * lv.gds[3]];
            }
        }
        a.g[i] = v;
    } else if (i < ng + nw) {
        const int64_t r = i - ng;
        const int j = (int)(r / a.co), c = (int)(r - (int64_t)j * a.co);
        a.wcr[r] = j < a.A ? a.w_cls[(int64_t)j * a.co + c] : (j < a.J ? a.w_reg[(int64_t)(j - a.A) * a.co + c] : 0.f);
    } else if (i < ng + nw + a.SP) {
        a.h[(i - ng - nw) * (a.co + 1) + a.co] = 1.f;
    }
}

// block (32 slots, 128 values of co): one 32 x 32 tile per wave, both products and the ReLU mask
__global__ void __launch_bounds__(kThreads) head_hidden_kernel(HeadArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, li = lane & 31;
    const int s0 = blockIdx.x * 32, c = blockIdx.y * 128 + wave * 32 + li;
    if (blockIdx.y * 128 + wave * 32 >= a.co) return;                       // wave-uniform
    const bool cok = c < a.co;
    const int cc = cok ? c : 0;
    f32x16 pre, d;
#pragma unroll
    for (int r = 0; r < 16; ++r) { pre[r] = 0.f; d[r] = 0.f; }
    tile_mac<false, true>(a.patchT + s0 + li, a.SP, true, a.w_conv + (int64_t)cc * a.K, 0, cok, 0, a.K, half, pre);
    tile_mac<true, false>(a.g + (int64_t)(s0 + li) * a.JP, 0, true, a.wcr + cc, a.co, cok, 0, a.JP, half, d);
    if (!cok) return;
    const float bias = a.b_conv ? a.b_conv[c] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int s = s0 + crow(r, half);
        const float p = pre[r] + bias;
        a.h[(int64_t)s * (a.co + 1) + c] = fmaxf(p, 0.f);
        a.dh[(int64_t)s * a.co + c] = p > 0.f ? d[r] : 0.f;
    }
}

// C[z][M][ldc] = A B over k in [z kper, min(K, (z + 1) kper)); block (128 columns, 32 rows, z)
template <bool KA, bool KB>
__global__ void __launch_bounds__(kThreads) head_gemm_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                             int64_t ldb, float* __restrict__ C, int64_t ldc, int M, int N, int K,
                                                             int kper) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, li = lane & 31;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 128 + wave * 32;
    if (n0 >= N) return;                                                    // wave-uniform
    const int row = m0 + li, col = n0 + li;
    const bool aok = row < M, bok = col < N;
    const int64_t ra = aok ? row : 0, cb = bok ? col : 0;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int k0 = blockIdx.z * kper, k1 = min(K, k0 + kper);
    tile_mac<KA, KB>(A + (KA ? ra * lda : ra), lda, aok, B + (KB ? cb * ldb : cb), ldb, bok, k0, k1, half, acc);
    if (!bok) return;
    float* out = C + (int64_t)blockIdx.z * M * ldc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + crow(r, half);
        if (m < M) out[(int64_t)m * ldc + col] = acc[r];
    }
}

// the partials [splits][rows][n + 1] in range order: rows < first go to (w0, b0), the rest up to `used` to (w1, b1); the last
// column is the bias gradient
__global__ void __launch_bounds__(kThreads) head_sum_kernel(const float* __restrict__ partial, int splits, int rows, int used, int n,
                                                            int first, float* __restrict__ w0, float* __restrict__ b0,
                                                            float* __restrict__ w1, float* __restrict__ b1) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x, n1 = n + 1, per = (int64_t)rows * n1;
    if (i >= (int64_t)used * n1) return;
    const int m = (int)(i / n1), c = (int)(i - m * n1);
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += partial[z * per + i];
    float* w = m < first ? w0 : w1;
    float* bb = m < first ? b0 : b1;
    const int r = m < first ? m : m - first;
    if (c < n) { if (w) w[(int64_t)r * n + c] = v; }
    else if (bb) bb[r] = v;
}

// block (slot, tap): the candidate writer of pixel q = p + (dy - 1, dx - 1)
__global__ void __launch_bounds__(kThreads) head_input_kernel(HeadArgs a) {
    const int s = blockIdx.x, tap = blockIdx.y;
    const int* o = a.slots + 4 * (int64_t)s;
    const int b = o[0], l = o[1];
    if (l < 0) return;
    const HeadLvl& lv = a.lv[l];
    const int qy = o[2] + tap / 3 - 1, qx = o[3] + tap % 3 - 1;
    if (qy < 0 || qy >= lv.H || qx < 0 || qx >= lv.W) return;
    const unsigned* own = a.owner + (int64_t)b * a.P + lv.pix_start;
    unsigned from[9], lowest = kNoOwner;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int py = qy - (t / 3 - 1), px = qx - (t % 3 - 1);
        from[t] = (py >= 0 && py < lv.H && px >= 0 && px < lv.W) ? own[py * lv.W + px] : kNoOwner;
        lowest = min(lowest, from[t]);
    }
    if (lowest != (unsigned)s) return;                                      // block-uniform: another candidate writes q
    float* dst = lv.g_feat + b * lv.gfs[0] + qy * lv.gfs[2] + qx * lv.gfs[3];
    for (int c = threadIdx.x; c < a.ci; c += kThreads) {
        float v = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t)
            if (from[t] != kNoOwner) v += a.T[(int64_t)from[t] * a.K + 9 * c + t];
        dst[c * lv.gfs[1]] = v;
    }
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct Plan { int SP, J, JP, K, splits, per; int64_t patchT, g, wcr, h, dh, T, p1, p2, total; };

bool make_plan(int S, int ci, int co, int A, Plan* p) {
    if (S < 1 || S > kMaxImages * 2 * kMaxNum || A < 1 || A > kMaxBase) return false;
    if (ci < 8 || co < 8 || ci > kMaxChannels || co > kMaxChannels || ci % 8 || co % 8) return false;
    p->SP = round_up(S, 32);
    p->J = 5 * A;
    p->JP = round_up(p->J, 8);
    p->K = 9 * ci;
    p->per = round_up((p->SP + kMaxSplits - 1) / kMaxSplits, 8);
    if (p->per < kMinPer) p->per = kMinPer;
    p->splits = (p->SP + p->per - 1) / p->per;
    int64_t at = 0;
    auto take = [&](int64_t n) { const int64_t o = at; at += (n + 3) / 4 * 4; return o; };       // 16-byte pieces
    p->patchT = take((int64_t)(p->K + 1) * p->SP);
    p->g = take((int64_t)p->SP * p->JP);
    p->wcr = take((int64_t)p->JP * co);
    p->h = take((int64_t)p->SP * (co + 1));
    p->dh = take((int64_t)p->SP * co);
    p->T = take((int64_t)p->SP * p->K);
    p->p1 = take((int64_t)p->splits * p->JP * (co + 1));
    p->p2 = take((int64_t)p->splits * co * (p->K + 1));
    p->total = at;
    return true;
}

}  // namespace

extern "C" {

int iif_rpn_sampled_pixels(const iif_rpn_grid* grid, int B, const int64_t* pos_inds, const int64_t* neg_inds, const int64_t* counts,
                           const float* pos_bbox_targets, int64_t num_expected_pos, int64_t num, int32_t* owner, int32_t* slots,
                           void* stream) {
    PixArgs a{};
    if (!fill_grid(grid, &a.g, nullptr) || !fill_lists(&a.s, B, pos_inds, neg_inds, counts, pos_bbox_targets, num_expected_pos, num))
        return IIF_EINVAL;
    int64_t P = 0;
    for (int l = 0; l < a.g.L; ++l) {
        a.pix_start[l] = (int)P;
        P += (int64_t)grid->W[l] * grid->H[l];
    }
    const int64_t total = (int64_t)B * (a.s.nep + a.s.num);
    if (total == 0) return IIF_OK;
    if (P < 1 || !owner || !slots || !aligned_to(owner, 4) || !aligned_to(slots, 4)) return IIF_EINVAL;
    a.P = (int)P;
    a.owner = reinterpret_cast<unsigned*>(owner);
    a.slots = slots;
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(owner, 0xff, (size_t)B * P * 4, st) != hipSuccess) return IIF_ELAUNCH;
    const dim3 grid_e((unsigned)cdiv64(total, kThreads));
    hipLaunchKernelGGL(pixels_mark_kernel, grid_e, dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(pixels_slots_kernel, grid_e, dim3(kThreads), 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

int64_t iif_rpn_head_sampled_workspace_bytes(int slots, int ci, int co, int num_base) {
    Plan p;
    return make_plan(slots, ci, co, num_base, &p) ? 4 * p.total : 0;
}

int iif_rpn_head_sampled_bwd(const iif_rpn_grid* grid, const iif_rpn_head_level* levels, int B, int slots_n, const int32_t* owner,
                             const int32_t* slots, const float* w_conv, const float* b_conv, const float* w_cls, const float* w_reg,
                             int ci, int co, float* d_w_conv, float* d_b_conv, float* d_w_cls, float* d_b_cls, float* d_w_reg,
                             float* d_b_reg, void* d_workspace, int64_t workspace_bytes, void* stream) {
    Grid g;
    Plan p;
    if (!levels || !fill_grid(grid, &g, nullptr) || B < 1 || B > kMaxImages) return IIF_EINVAL;
    const int A = grid->num_base[0];
    for (int l = 1; l < g.L; ++l)
        if (grid->num_base[l] != A) return IIF_EUNSUPPORTED;
    if (ci < 1 || co < 1 || slots_n < 1) return IIF_EINVAL;
    if (!make_plan(slots_n, ci, co, A, &p)) return IIF_EUNSUPPORTED;
    if (!owner || !slots || !w_conv || !w_cls || !w_reg || !d_workspace || workspace_bytes < 4 * p.total) return IIF_EINVAL;
    if (!aligned_to(owner, 4) || !aligned_to(slots, 4) || !aligned_to(b_conv, 4) || !aligned_to(w_cls, 4) || !aligned_to(w_reg, 4) ||
        !aligned_to(d_w_conv, 4) || !aligned_to(d_b_conv, 4) || !aligned_to(d_w_cls, 4) || !aligned_to(d_b_cls, 4) ||
        !aligned_to(d_w_reg, 4) || !aligned_to(d_b_reg, 4))
        return IIF_EINVAL;
    if (!aligned_to(w_conv, 16) || !aligned_to(d_workspace, 16)) return IIF_EUNSUPPORTED;   // rows of 9 Ci floats are read 16 bytes at a time
    HeadArgs a{};
    int64_t P = 0;
    bool want_input = false;
    for (int l = 0; l < g.L; ++l) {
        const iif_rpn_head_level& m = levels[l];
        HeadLvl& o = a.lv[l];
        o.H = grid->H[l]; o.W = grid->W[l]; o.pix_start = (int)P;
        P += (int64_t)o.H * o.W;
        const bool empty = o.H == 0 || o.W == 0;
        if (!empty && (!m.feat || !m.grad_scores || !m.grad_deltas)) return IIF_EINVAL;
        if (l == 0) want_input = m.grad_feat != nullptr;
        if ((m.grad_feat != nullptr) != want_input) return IIF_EINVAL;     // the gradient of every level's features, or of none
        if (!aligned_to(m.feat, 4) || !aligned_to(m.grad_feat, 4) || !aligned_to(m.grad_scores, 4) || !aligned_to(m.grad_deltas, 4))
            return IIF_EINVAL;
        o.feat = m.feat; o.g_feat = m.grad_feat; o.g_scores = m.grad_scores; o.g_deltas = m.grad_deltas;
        for (int k = 0; k < 4; ++k) {
            if (m.feat_strides[k] < 0 || m.grad_feat_strides[k] < 0 || m.grad_score_strides[k] < 0 || m.grad_delta_strides[k] < 0)
                return IIF_EINVAL;
            o.fs[k] = m.feat_strides[k]; o.gfs[k] = m.grad_feat_strides[k];
            o.gss[k] = m.grad_score_strides[k]; o.gds[k] = m.grad_delta_strides[k];
        }
    }
    if (P < 1) return IIF_EINVAL;
    float* ws = static_cast<float*>(d_workspace);
    a.L = g.L; a.P = (int)P; a.S = slots_n; a.SP = p.SP; a.A = A; a.J = p.J; a.JP = p.JP; a.ci = ci; a.co = co; a.K = p.K;
    a.owner = reinterpret_cast<const unsigned*>(owner); a.slots = slots;
    a.w_conv = w_conv; a.b_conv = b_conv; a.w_cls = w_cls; a.w_reg = w_reg;
    a.patchT = ws + p.patchT; a.g = ws + p.g; a.wcr = ws + p.wcr; a.h = ws + p.h; a.dh = ws + p.dh; a.T = ws + p.T;
    float* p1 = ws + p.p1;
    float* p2 = ws + p.p2;
    hipStream_t st = as_stream(stream);
    const dim3 blk(kThreads);
    hipLaunchKernelGGL(head_patch_kernel, dim3(p.SP / 64 + (p.SP % 64 ? 1 : 0), (p.K + 1 + 63) / 64), blk, 0, st, a);
    IIF_LAUNCH_CHECK();
    const int64_t prep = (int64_t)p.SP * p.JP + (int64_t)p.JP * co + p.SP;
    hipLaunchKernelGGL(head_prep_kernel, dim3((unsigned)cdiv64(prep, kThreads)), blk, 0, st, a);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_hidden_kernel, dim3(p.SP / 32, (co + 127) / 128), blk, 0, st, a);
    IIF_LAUNCH_CHECK();
    if (d_w_cls || d_b_cls || d_w_reg || d_b_reg) {      // [dW_cls; dW_reg | db] [JP][co + 1] = g^T [h | 1], slots in ranges
        hipLaunchKernelGGL((head_gemm_kernel<false, false>), dim3((co + 1 + 127) / 128, (p.JP + 31) / 32, p.splits), blk, 0, st, a.g,
                           (int64_t)p.JP, a.h, (int64_t)(co + 1), p1, (int64_t)(co + 1), p.JP, co + 1, p.SP, p.per);
        IIF_LAUNCH_CHECK();
        hipLaunchKernelGGL(head_sum_kernel, dim3((unsigned)cdiv64((int64_t)p.J * (co + 1), kThreads)), blk, 0, st, p1, p.splits, p.JP,
                           p.J, co, A, d_w_cls, d_b_cls, d_w_reg, d_b_reg);
        IIF_LAUNCH_CHECK();
    }
    if (d_w_conv || d_b_conv) {                          // [dW_conv | db_conv] [co][K + 1] = dh^T [patch | 1]
        hipLaunchKernelGGL((head_gemm_kernel<false, true>), dim3((p.K + 1 + 127) / 128, (co + 31) / 32, p.splits), blk, 0, st, a.dh,
                           (int64_t)co, a.patchT, (int64_t)p.SP, p2, (int64_t)(p.K + 1), co, p.K + 1, p.SP, p.per);
        IIF_LAUNCH_CHECK();
        hipLaunchKernelGGL(head_sum_kernel, dim3((unsigned)cdiv64((int64_t)co * (p.K + 1), kThreads)), blk, 0, st, p2, p.splits, co, co,
                           p.K, co, d_w_conv, d_b_conv, (float*)nullptr, (float*)nullptr);
        IIF_LAUNCH_CHECK();
    }
    if (!want_input) return IIF_OK;
    // T [SP][K] = dh W_conv
    hipLaunchKernelGGL((head_gemm_kernel<true, false>), dim3((p.K + 127) / 128, p.SP / 32, 1), blk, 0, st, a.dh, (int64_t)co, w_conv,
                       (int64_t)p.K, a.T, (int64_t)p.K, p.SP, p.K, co, co);
    IIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_input_kernel, dim3(slots_n, 9), blk, 0, st, a);
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}

}  // extern "C"
