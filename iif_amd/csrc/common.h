// Shared device helpers for the gfx950 kernels (wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/iif_amd.h"

#define IIF_WAVE 64

#define IIF_LAUNCH_CHECK()                          \
    do {                                            \
        hipError_t e__ = hipGetLastError();         \
        if (e__ != hipSuccess) return IIF_ELAUNCH;  \
    } while (0)

// LDS-DMA addressing is a 32-bit byte offset with a hardware range check: an operand read through it stays below this many bytes
constexpr long long kDmaRange = 0x7f000000LL;

// Kernel families of the convolution entry.  0 .. 11 are public (iif_conv_affine_route returns them); the rest are internal.
enum { IIF_ROUTE_NONE = 0, IIF_ROUTE_TILE = 1, IIF_ROUTE_TILE_2STAGE = 2, IIF_ROUTE_TILE_GENERAL = 3, IIF_ROUTE_TILE256 = 4,
       IIF_ROUTE_HALO = 5, IIF_ROUTE_FRAG = 6, IIF_ROUTE_FRAG_G16 = 7, IIF_ROUTE_STREAM1X1 = 8, IIF_ROUTE_REGW1X1 = 9,
       IIF_ROUTE_REGW3X3 = 10, IIF_ROUTE_REGSTAGE = 11, IIF_ROUTE_STEM = 12, IIF_ROUTE_TILE_MC = 13 };

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;

__device__ __forceinline__ float bf16_bits_to_f32(unsigned int lo16) {
    return __uint_as_float(lo16 << 16);
}
// round-to-nearest-even through the compiler's cast (v_cvt_pk_bf16_f32; keeps NaN a NaN)
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ unsigned int pack_bf16x2(float lo, float hi) {
    return (unsigned int)f32_to_bf16_bits(lo) | ((unsigned int)f32_to_bf16_bits(hi) << 16);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

static inline hipStream_t as_stream(void* s) { return (hipStream_t)s; }
static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline bool aligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
static inline bool aligned_to(const void* p, unsigned n) { return aligned(p, (int)n); }     // the head-side entries' spelling

// ---- The convolution entry in two steps (conv_igemm.hip; continuations in conv_regw.hip and conv_stem.hip): SELECT maps a
// ConvSel - the geometry and WHICH operands a call has, no addresses - to a ConvRoute or a status code on the host alone;
// LAUNCH runs exactly the selected kernel on the operands of the ConvCall.

// One call of the entry: zero-initialise, then set fields by name.
struct ConvCall {
    const iif_conv_desc* d; const void* src; const void* wgt; void* dst; const void* res; const unsigned char* res_bits; const float* bias;
    float* bn_partial; int64_t bn_cap; int32_t* n_partials; void* stream;
    const void* bw_x; const unsigned char* bw_bits; const float* bw_stats;     // (read with bn_partial only)
    int mask_store; const void* src2; int cs2; const float* sbias; int no_store;
    const float* aff; const float* aff2; unsigned char* relu_out;
    int aff_any;                      // aff on every geometry the staged epilogue serves (iif_conv_igemm_affine)
    const void* rx_src2; const void* rx_w3; int rx_k2, rx_ldw3;
    const float* pro_stats; void* pro_out; unsigned char* pro_bits; float* pro_csum;
    float* pg_slab; long long pg_cap; int pg_ld; int* pg_count;
};

// What selection reads.  Geometry as in ConvArgs (Hd / Wd / M / ntaps / in_shift / scatter: of ONE launch - the parity classes of
// a stride-2 data gradient are launches of their own); a bool named like an operand says that the call has it.
struct ConvSel {
    int N, Hs, Ws, Cs, Hd, Wd, Cd, R, S, sshift, pad, transposed, ldw, M, groups, spitch, dpitch, Cs2, esz;
    bool outf32;
    long long src_bytes, wgt_bytes;   // wgt_bytes: one group's weight matrix
    bool res, res_bits, bias, bn_partial, bw_x, bw_bits, bw_stats, src2, sbias, aff, aff2, relu_out, rx_src2, rx_w3, pro_stats, pg_slab,
         pg_count, wfrag;
    bool res_is_dst, pg_unaligned;    // the residual is the destination (dst += ...); pg_slab is not 16-byte aligned
    int mask_store, no_store, wfrag_kind, rx_k2, rx_ldw3, pg_ld, bn_row0;
    long long bn_cap, pg_cap;
    int ntaps, in_shift, scatter;
};

struct ConvRoute {
    int family;                       // IIF_ROUTE_*
    // instance within the family: register-weight 1x1 -> index of (K, CW, MT, EPI, K2, PRO, PG) in conv_regw.hip's list; register-
    // weight 3x3 -> its EPI; streaming -> BN (256: K 64, else K 256); halo -> rows per tile; tile families -> columns per tile
    int inst;
    int cls;                          // parity class 2 py + px of a stride-2 data gradient launched class by class, else -1
    int mtiles, ntiles;
    unsigned grid, grid_y, block;
    int rows, slabs;                  // partial rows (bn_row0 onwards) and P / Gram slabs the launch writes
};

// `rows` partial rows from a.bn_row0 must fit the caller's buffer
inline int iif_claim_rows(const ConvSel& a, ConvRoute* r, int rows) {
    r->rows = 0;
    if (!a.bn_partial) return IIF_OK;
    if ((long long)(a.bn_row0 + rows) * 2 * a.dpitch > a.bn_cap) return IIF_EINVAL;
    r->rows = rows;
    return IIF_OK;
}

// The selectors of the other files return IIF_OK with *r filled, IIF_EUNSUPPORTED where the family does not take the launch (the
// caller goes on to the next one) or IIF_EINVAL; a launch function runs the selected instance and cannot refuse.

// conv_stem.hip: the space-to-depth stem (4 x 4 taps over 16 padded channels -> 64, bf16) with BN partial sums
bool iif_stem4x4_geometry(const ConvSel& a);      // the layer's shape (its image size aside)
int iif_stem4x4_select(const ConvSel& a, ConvRoute* r);
int iif_stem4x4_launch(const ConvRoute& r, const ConvCall& c, const ConvSel& a, hipStream_t st);

// conv_regw.hip: 1x1 / stride 1 forward or data gradient with the weights in registers (narrow -> wide layers), bf16, BN partial
// sums.  Modes of the selector:
//   IIF_REGW_PLAIN  plain store or the data-gradient options of staged_drain (residual / its bits / gated store / upstream sums; with
//                   rx_*: the upstream x recomputed per tile from the upstream block's a2 [M, rx_k2] and its conv3 weights
//                   [N, rx_ldw3]; with pg_*: P = dst^T a2 and Gram = a2^T a2 as by-products, one fp32 slab [(N + rx_k2), pg_ld] per
//                   tile sequence - iif_slab_sum adds them up); with pro_*: `src` is the raw output of the previous convolution, its
//                   BN + ReLU (stats laid out as iif_bn_finalize_stats writes them) is applied to each tile in LDS and the activation
//                   written out as a by-product (out [M, K] bf16, bits one byte per 16-byte vector; csum nullable: one row [2][K] =
//                   (column sums of the activation, zeros) per partial row of the launch: iif_bn_partial_sums reduces them)
//   IIF_REGW_FWDBN / IIF_REGW_STATS  the two passes of the never-stored conv + BN (+ identity / normalised shortcut) + ReLU forward
//                   (K in {64, 128, 256}, N a multiple of 256): the convolution with bn_apply's arithmetic in its epilogue, and the
//                   statistics from the accumulators (no store; optionally with the prologue)
enum { IIF_REGW_PLAIN = 0, IIF_REGW_FWDBN = 2, IIF_REGW_STATS = 3 };
bool iif_dense1x1(const ConvSel& a);              // bf16 1x1 / stride 1 / pad 0, dense, one grid: the geometry these kernels cover
bool iif_regw1x1_ok(int M, int K, int N, int epi);
bool iif_regw1x1_rx_ok(int M, int K, int N, int k2);
bool iif_regw1x1_pg_ok(int M, int K, int N, int k2);      // ... with the P / Gram by-product (one N slice, k2 = 64)
bool iif_regw1x1_pro_ok(int M, int K, int N);
bool iif_regw1x1_fwdbn_ok(int M, int K, int N);
int iif_regw1x1_select(const ConvSel& a, int mode, ConvRoute* r);
int iif_regw1x1_launch(const ConvRoute& r, const ConvCall& c, const ConvSel& a, hipStream_t st);
// 3x3 / stride 1 / pad 1, C -> C channels (64), forward or data gradient (explicit tap list), optional upstream BN-backward sums;
// aff (forward, no sums): dst = relu(fmaf(a, bf16(conv), b) + r), r = nothing | res | fmaf(a2, res, b2), the coefficient rows of
// iif_bn_apply; relu_out nullable
int iif_regw3x3_select(const ConvSel& a, ConvRoute* r);
int iif_regw3x3_launch(const ConvRoute& r, const ConvCall& c, const ConvSel& a, const signed char* tap_dy, const signed char* tap_dx,
                       const unsigned char* tap_w, hipStream_t st);

// Test switches of the convolution files (this is the whole list; INTEGRATION.md, "Environment switches", says what each is for), read from the environment ONCE;
// iif_conv_reload_env() re-reads them (tests flip them between calls).
//   IIF_CONV_REGSTAGE        every launch on the register-staged kernels (the fallback for operands >= 2 GiB)
//   IIF_CONV_NO_STREAM1X1    no launch on the persistent streaming 1x1 kernel;  IIF_CONV_STREAM1X1_FORCE: every shape it has a
//                            plan for, small grids and data gradients included (default: three forward shapes, see use_stream1x1)
//   IIF_CONV_NO_HALO / IIF_CONV_HALO_FORCE   3x3 halo kernel off / also on small grids
//   IIF_CONV_NO_V2 / IIF_CONV_V2_FORCE       3x3 fragment kernel (64 channels) off / also on small grids
//   IIF_CONV_NO_REGW / IIF_CONV_NO_REGW_FWDBN  register-weight kernels off / their BN-epilogue passes off (tests: on the tile kernels)
//   IIF_CONV_NO_BM256_2SRC   see use_bm256;  IIF_REGW_K512_CW16 / IIF_REGW_NO_X2 / IIF_REGW_K512_NO_EPI: see regw_plan
struct ConvSwitches {
    bool no_stream, force_stream, regstage, no_v2, no_halo, force_halo, v2_force, no_regw, no_regw_fwdbn, no_bm256_2src,
         regw_k512_cw16, regw_no_x2, regw_k512_no_epi;
    static ConvSwitches read();
};
extern ConvSwitches g_sw;

// Compute units a persistent grid (one or two resident blocks per CU: conv_regw.hip, conv_stem.hip, the streaming 1x1 kernel)
// sizes itself to: the device's count, or the budget set by iif_set_cu_budget() when that is smaller (a rank that overlaps
// RCCL's reduction kernels with backward leaves them a few CUs instead of making their blocks queue behind a persistent grid).
int iif_persistent_cus();
int iif_persistent_grid(int unit);      // blocks of a grid launched in whole units of `unit` blocks, within the budget (see iif_host.cpp)
