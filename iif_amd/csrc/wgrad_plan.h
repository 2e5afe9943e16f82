// The split-K decision of a weight-gradient launch as a value: kernel family and tile, K steps, the number of splits (the
// requested or the automatic round, cut to the workspace and to the work), steps per split, blocks launched, and the form of
// the slab reduction.  Every launcher of conv_wgrad.hip takes its numbers from here, and so does the planning query
// iif_conv_wgrad_plan, which launches nothing: a test asks the query which kernel and how many splits a call gets instead of
// repeating the arithmetic.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "../../include/iif_amd.h"

namespace iif_plan {

// what the decision reads of a launch (iif_conv_wgrad's descriptor, or iif_wgrad1x1_stacked's arguments as a 1x1 descriptor)
struct WgShape {
    int N, Hs, Ws, Cs, Hd, Wd, Cd, R, S, sshift, pad, ldw, M, K, groups, xpitch, ypitch;
    int esz;                    // operand element bytes: 2 (bf16) or 4 (fp32)
    int cd2;                    // stacked 1x1: channels of the second gradient tensor (Cd = cd1 + cd2); 0 otherwise
    bool stacked, gram;         // iif_wgrad1x1_stacked; x and dy are one tensor (the Gram matrix)
    int64_t x_bytes, dy_bytes;
};

struct WgPlan {
    int rc;                     // IIF_OK, or the status the launch returns before launching anything
    int family;                 // IIF_WGRAD_*
    int bc, bnw;                // output-channel tile, input-column tile
    int ktiles, ntiles, tiles;  // (nine-tap: ktiles = co_tiles, ntiles = ci_tiles)
    int nsteps, splits, steps_per_split;
    int64_t blocks;             // workgroups of the product launch (the padded grid included)
    int rows;                   // slab rows; slab = rows * ldw floats
    int64_t slab;
    int stages, nch;            // slab reduction: 0 (one split, none), 1 (one pass), 2 (chunks of 16, then the nch chunk sums)
    int reduce_blocks;
    int HB, LB, LEAD;           // nine-tap ring lead; stem window blocks
};

inline int share_of(int splits_req) { return splits_req < 0 ? -splits_req : 1; }

// sum of `splits` slabs of `slab` floats: one pass, or - few elements x many slabs - chunks of 16 slabs summed in parallel
// into a stage area BEHIND the slabs (nch more slabs of workspace), then one pass over the nch chunk sums
struct ReducePlan { int blocks, stages, nch; };
inline ReducePlan reduce_plan(int splits, int64_t slab, int64_t ws_bytes) {
    const int64_t total4 = slab / 4, b = (total4 + 255) / 256;
    ReducePlan r{(int)(b < 2048 ? b : 2048), 1, 0};
    if (splits > 32 && r.blocks * 256 < 65536) {
        const int nch = (splits + 15) / 16;
        if ((int64_t)(splits + nch) * slab * 4 <= ws_bytes) { r.stages = 2; r.nch = nch; }
    }
    return r;
}

// the automatic round is `splits`; cut it to the workspace and the work, even the splits out, plan the reduction
inline void wg_finish(WgPlan& p, int splits, int ldw, int64_t ws_bytes, int64_t blocks_per_split8, bool pad8) {
    p.slab = (int64_t)p.rows * ldw;
    const int64_t fit = ws_bytes / (p.slab * 4);
    if (splits > fit) splits = (int)fit;
    if (splits < 1) splits = 1;
    if (splits > p.nsteps) splits = p.nsteps > 0 ? p.nsteps : 1;
    if (splits > 65535) splits = 65535;
    p.steps_per_split = (p.nsteps + splits - 1) / splits;
    splits = (p.nsteps + p.steps_per_split - 1) / p.steps_per_split;
    if (splits < 1) splits = 1;
    p.splits = splits;
    p.blocks = blocks_per_split8 * (pad8 ? (splits + 7) / 8 * 8 : splits);
    p.stages = 0; p.nch = 0; p.reduce_blocks = 0;
    if (splits > 1) {
        const ReducePlan r = reduce_plan(splits, p.slab, ws_bytes);
        p.stages = r.stages; p.nch = r.nch; p.reduce_blocks = r.blocks;
    }
}

inline int max_by_work(int nsteps) { return nsteps / 8 > 0 ? nsteps / 8 : 1; }

// all nine taps per block (conv3x3_wgrad_halo_kernel); false: beyond the 32-bit virtual index, the caller falls back
inline bool wg_plan_halo(const WgShape& a, int64_t ws_bytes, int splits_req, WgPlan& p) {
    const bool grouped = a.groups > 1;
    p.family = IIF_WGRAD_NINETAP; p.bc = 64; p.bnw = 64;
    p.ntiles = grouped ? a.groups : a.Cs / 64; p.ktiles = grouped ? 1 : a.Cd / 64;
    p.HB = a.Wd + 3 <= 32 ? 32 : 64;
    const int64_t vt = (int64_t)a.N * (a.Hd + 2) * (a.Wd + 2);
    if (vt > 0x7fff0000LL) return false;
    p.nsteps = (int)((vt + 31) / 32);
    p.tiles = p.ntiles * p.ktiles;
    int splits = splits_req;
    if (splits <= 0) {
        const int per_cu = 2;
        // grouped layers (ResNeXt: the weight gradient is block-diagonal, 8 chunks x 147 KB at 14 x 14 against 51 MB of operands) take
        // a quarter of a round: ResNeXt-101 20.80 / 20.87 (full) -> 20.37 (half) -> 20.36 / 20.29 (quarter) -> 21.0 (eighth) ms per step;
        // dense layers keep the full round (ResNet-50: 16.57 -> 16.65 with half)
        static const int halo_div = [] { const char* e = getenv("IIF_WGRAD_HALO_DIV"); return e ? atoi(e) : 1; }();
        static const int halo_gdiv = [] { const char* e = getenv("IIF_WGRAD_HALO_GROUPED_DIV"); return e ? atoi(e) : 4; }();
        const int hdiv = grouped ? halo_gdiv : halo_div;
        splits = 256 * per_cu / share_of(splits_req) / p.tiles / (hdiv > 0 ? hdiv : 1);
        if (splits < 1) splits = 1;
        if (splits > max_by_work(p.nsteps)) splits = max_by_work(p.nsteps);
    }
    p.rows = a.groups * a.Cd;
    wg_finish(p, splits, a.ldw, ws_bytes, p.tiles, true);
    return true;
}

// all sixteen taps per block for the space-to-depth stem (conv4x4_s2d_wgrad_kernel); false: the caller falls back
inline bool wg_plan_stem(const WgShape& a, int64_t ws_bytes, int splits_req, WgPlan& p) {
    p.family = IIF_WGRAD_STEM; p.bc = 64; p.bnw = 256; p.ktiles = p.ntiles = p.tiles = 1;
    const int Wp = a.Wd + 3;
    p.LB = (2 * Wp + 2 + 31) / 32;
    p.LEAD = p.LB + (31 + Wp + 1) / 32;
    if (p.LEAD + 2 > 14) return false;               // the 16-block x ring cannot hold the window
    const int64_t vt = (int64_t)a.N * (a.Hd + 3) * Wp;
    if (vt > 0x7fff0000LL) return false;
    p.nsteps = (int)((vt + 31) / 32);
    int splits = splits_req;
    if (splits <= 0) {
        const int per_cu = 2;
        splits = 256 * per_cu / share_of(splits_req);
        if (splits > max_by_work(p.nsteps)) splits = max_by_work(p.nsteps);
    }
    p.rows = a.Cd;
    wg_finish(p, splits, a.ldw, ws_bytes, 1, true);
    return true;
}

// 1x1 / stride 1 (wgrad1x1_body): tile by the channel counts, one co-resident round of splits
inline void wg_plan_1x1(const WgShape& g, int64_t ws_bytes, int splits_req, WgPlan& p) {
    p.family = IIF_WGRAD_1X1;
    const int cd1 = g.Cd - g.cd2;
    // (stacked: the first tensor's channels fill whole tiles; the second's last tile may be partly empty)
    const int bc = g.stacked ? (cd1 % 256 == 0 ? 256 : 128) : ((g.Cd >= 256 && g.Cd % 256 == 0) ? 256 : (g.Cd <= 64 ? 64 : 128));
    static const bool no_wide = getenv("IIF_WGRAD_NO_64X256") != nullptr;
    const int bnw = (g.Cs <= 64 && bc == 64) ? 64 : ((bc == 64 && g.Cs > 128 && g.Cs % 256 == 0 && !no_wide) ? 256 : 128);      // (256 x 64 as two 4-wave blocks per CU was slower than 256 x 128 with half of its columns empty: 0.115 against 0.106 ms at 56 x 56)
    p.bc = bc; p.bnw = bnw;
    p.ktiles = (g.Cd + bc - 1) / bc;
    p.ntiles = (g.Cs + bnw - 1) / bnw;
    p.nsteps = (g.M + 31) / 32;
    p.tiles = p.ktiles * p.ntiles;
    // blocks per CU by LDS (3 stages of 32 x (bnw + bc) x 2 bytes) and registers: 256 x 128: one 8-wave block (72 KB);
    // 128 x 128: three (48 KB); 64 x {128, 64}: four
    const int per_cu = bc == 256 ? 1 : (bc == 128 ? 3 : (bnw == 256 ? 2 : 4));
    int splits = splits_req;
    const int64_t slab = (int64_t)g.Cd * g.ldw;
    if (splits <= 0) {
        splits = 256 * per_cu / share_of(splits_req) / p.tiles;
        if (splits < 1) splits = 1;
        if (splits > max_by_work(p.nsteps)) splits = max_by_work(p.nsteps);
        // Small outputs write splits x their own size in slabs: a Gram matrix a2^T a2 (16-256 KB) 16-48 MB, P = g~^T a2 of the
        // 56 x 56 stage (64 KB) 16 MB - more than the operands at 14 x 14.  Round 5, same-call A/B of the step (ms): default splits
        // 18.02; Gram 1/4 + other outputs <= 256 KB 1/2: 17.78; Gram 1/8: 17.77; 1/2 for EVERY 1x1 weight gradient 17.86 and for
        // the nine-tap kernel 17.90 (their streams become the critical path).  Gram (x == dy) is forward data a block ahead on the
        // shortcut stream: nothing waits for it.  IIF_WGRAD_GRAM_DIV / IIF_WGRAD_SMALL_DIV = 1 restore the full round of splits.
        static const int small_div = [] { const char* e = getenv("IIF_WGRAD_SMALL_DIV"); return e ? atoi(e) : 2; }();
        static const int gram_div = [] { const char* e = getenv("IIF_WGRAD_GRAM_DIV"); return e ? atoi(e) : 8; }();
        const bool gram = g.gram && !g.stacked;
        static const int small_kb = [] { const char* e = getenv("IIF_WGRAD_SMALL_KB"); return e ? atoi(e) : 256; }();
        // (late round 6: outputs up to 4 MB - the 14 x 14 / 7 x 7 1x1 layers - take half a round too: 16.75 / 16.80 / 16.84 -> 16.73 / 16.71 /
        // 16.78 ms per step in one call, their slabs halved; a quarter round: 17.2.  IIF_WGRAD_MID_DIV=1 restores the full round)
        static const int mid_div = [] { const char* e = getenv("IIF_WGRAD_MID_DIV"); return e ? atoi(e) : 2; }();
        const int div = gram ? gram_div : (slab * 4 <= ((int64_t)small_kb << 10) ? small_div : (slab * 4 <= (4 << 20) ? mid_div : 1));
        if (div > 1 && splits > 8) { splits /= div; if (splits < 8) splits = 8; }       // (never more splits than before)
    }
    p.rows = g.Cd;
    wg_finish(p, splits, g.ldw, ws_bytes, p.tiles, true);
}

// one tap-and-channel tile per block: the LDS-DMA kernel (conv_wgrad_dma_kernel) or, for operands beyond the 32-bit byte
// offsets and under IIF_CONV_REGSTAGE, the register-staged one (conv_wgrad_kernel)
inline void wg_plan_generic(const WgShape& a, bool dma_ok, int64_t ws_bytes, int splits_req, WgPlan& p) {
    const int ROWS = a.esz == 2 ? 32 : 16;
    // 256-channel tiles (8 waves): bf16, dense, >= 256 output channels, the LDS-DMA path
    const bool wide = a.esz == 2 && dma_ok && a.groups == 1 && a.Cd >= 256 && a.Cd % 256 == 0;
    const int bc = wide ? 256 : (a.Cd <= 64 ? 64 : 128);
    p.family = dma_ok ? IIF_WGRAD_DMA : IIF_WGRAD_REGSTAGE;
    p.bc = bc; p.bnw = 128;
    p.ktiles = (a.Cd + bc - 1) / bc;
    p.ntiles = (a.K + 127) / 128;
    p.nsteps = (a.M + ROWS - 1) / ROWS;
    p.tiles = p.ktiles * p.ntiles;
    int splits = splits_req;
    if (splits <= 0) {
        // one full co-resident round: 256 CUs x (3 | 4) workgroups (LDS 48 | 36 KB each), so every
        // workgroup gets the same number of steps and there is no tail round
        // blocks per CU: 4 (64-channel tile), 3 (128), and ONE 8-wave block for the 256-channel tile: two per CU write twice
        // the split-K slabs for nothing (step 20.67 -> 20.62 ms at one; 0.75 / 1.25 per CU leave a tail round: 21.2 / 20.8;
        // round 3, scripts removed).
        const int slots = 256 * (bc == 256 ? 1 : (bc == 128 ? 3 : 4)) / share_of(splits_req);
        splits = slots / (p.tiles * a.groups);
        if (splits < 1) splits = 1;
        if (splits > max_by_work(p.nsteps)) splits = max_by_work(p.nsteps);
    }
    p.rows = a.groups * a.Cd;
    // (the register-staged kernel takes grid (tiles, splits); the LDS-DMA kernel a padded 1-D grid per group)
    wg_finish(p, splits, a.ldw, ws_bytes, dma_ok ? (int64_t)p.tiles * a.groups : p.tiles, dma_ok);
    if (a.groups > 1 && !dma_ok) p.rc = IIF_EUNSUPPORTED;
}

// the whole decision of iif_conv_wgrad / iif_wgrad1x1_stacked.  ws_bytes: bytes of workspace (0 without one).
inline WgPlan wgrad_plan(const WgShape& a, int64_t ws_bytes, int splits_req) {
    WgPlan p{};
    p.rc = IIF_OK;
    if (a.stacked) { wg_plan_1x1(a, ws_bytes, splits_req, p); return p; }
    // (IIF_CONV_REGSTAGE: every launch on the register-staged kernel, the fallback for operands >= 2 GiB; tests)
    const bool force_v1 = getenv("IIF_CONV_REGSTAGE") != nullptr;       // (read per call: a test flips it)
    const bool dma_ok = !force_v1 && a.x_bytes < 0x7ffffff0LL && a.dy_bytes < 0x7ffffff0LL;
    if (a.esz == 2) {
        // dense: channels in 64s; grouped: 64-channel chunks (the nine-tap tile IS a chunk)
        const bool shape = a.groups == 1 ? (a.Cs % 64 == 0 && a.Cd % 64 == 0 && a.xpitch == a.Cs && a.ypitch == a.Cd)
                                         : (a.Cs == 64 && a.Cd == 64 && a.ldw >= 576);
        const bool halo = dma_ok && shape && a.R == 3 && a.S == 3 && a.sshift == 0 && a.pad == 1 && a.Hs == a.Hd &&
                          a.Ws == a.Wd && a.Wd + 3 <= 64;
        if (halo && wg_plan_halo(a, ws_bytes, splits_req, p)) return p;
        const bool stem = dma_ok && a.groups == 1 && a.R == 4 && a.S == 4 && a.sshift == 0 && a.pad == 2 && a.Hs == a.Hd &&
                          a.Ws == a.Wd && a.Cs == 16 && a.Cd == 64 && a.xpitch == 16 && a.ypitch == 64;
        if (stem && wg_plan_stem(a, ws_bytes, splits_req, p)) return p;
        if (dma_ok && a.R == 1 && a.S == 1 && a.sshift == 0 && a.pad == 0 && a.groups == 1 && a.Hs == a.Hd && a.Ws == a.Wd &&
            a.xpitch == a.Cs && a.ypitch == a.Cd) {
            wg_plan_1x1(a, ws_bytes, splits_req, p);
            return p;
        }
    }
    p = WgPlan{};
    p.rc = IIF_OK;
    wg_plan_generic(a, dma_ok, ws_bytes, splits_req, p);
    return p;
}

}  // namespace iif_plan
