// Launch decisions of the streaming kernels that depend on nothing but the SIZE of the tensor: grid, per-thread unroll, rows per
// block.  Every launch calls these functions, and so does the planning query iif_stream_plan (pool_misc.hip), which launches
// nothing: a test asks the query on which side of a threshold its tensor falls instead of repeating the arithmetic.
#pragma once
#include <stdint.h>
#include <stdlib.h>

namespace iif_plan {

// grid of the two BN normalisation passes: one trip per thread over U vectors (U = 4 where that still leaves >= 2 048 blocks).
// In the ResNet-50 step (same-call A/B, ms per step): round 4's form (4 096 blocks looping, U = 1) 18.59 / 18.62; one trip,
// U <= 4 18.32 / 18.33; the same with non-temporal stores 18.34 / 18.41 (alone they are the faster form, 6.6 against 6.2 TB/s;
// in the step the consumer reads the tensor next); U = 1 one trip 19.09 / 19.04 (100 k blocks of one vector per thread: alone
// 6.1 TB/s, in the step the other streams' blocks wait behind them); a grid capped at 4 096 / 2 048 / 1 024 blocks with U <= 4
// 18.42 / 18.47 / 18.51.  IIF_BN_GRID_CAP=<blocks>, IIF_BN_UNROLL=<1|2|4>, IIF_BN_NT_STORES=1 select the other forms (read
// once per process).
struct StreamGrid { int blocks, u; bool nts; };
inline StreamGrid stream_grid(int64_t total_vec) {
    static const int64_t cap = [] { const char* e = getenv("IIF_BN_GRID_CAP"); return e ? atoll(e) : (1LL << 30); }();
    static const bool nts = getenv("IIF_BN_NT_STORES") != nullptr;
    static const int umax = [] { const char* e = getenv("IIF_BN_UNROLL"); return e ? atoi(e) : 4; }();
    int u = total_vec >= (int64_t)4 * 256 * 2048 ? 4 : (total_vec >= (int64_t)2 * 256 * 2048 ? 2 : 1);
    if (u > umax) u = umax;
    const int64_t b = (total_vec + 256 * u - 1) / (256 * u);
    return StreamGrid{(int)(b < cap ? b : cap), u, nts};
}

// grid-stride kernels of pool_misc.hip (one work item per thread and trip) and the RMSprop step: at most 8 192 blocks
inline int sblocks(int64_t n) { const int64_t b = (n + 255) / 256; return (int)(b < 8192 ? (b > 0 ? b : 1) : 8192); }
inline int rms_blocks(int64_t n4) { return sblocks(n4); }

// the two per-vector passes of se.hip: at most 4 096 blocks
inline unsigned se_stream_blocks(int64_t total) {
    int64_t b = (total + 255) / 256;
    if (b > 256 * 16) b = 256 * 16;
    return (unsigned)(b < 1 ? 1 : b);
}

// fused stem pool (iif_maxpool_bn_forward, 3 x 3 / 2 / 1): one pooled row per block pass, at most 16 384 blocks
inline int pool_row_blocks(int64_t rows) { return (int)(rows < 16384 ? rows : 16384); }

// iif_bn_backward_pool_fused: image rows per block (8; more where a row is narrow, so that a block has >= 2 048 vectors), the
// number of row groups = blocks, and whether the blocks are dealt round the 8 XCDs (only a whole number of eighths is)
struct PoolFusedGrid { int rows_per_block, groups; bool remap; };
__host__ __device__ inline bool pool_fused_remap(unsigned groups) { return (groups & 7u) == 0; }
inline PoolFusedGrid pool_fused_grid(int total_rows, int w, int cv) {
    int rpb = 8;                     // rows per block: 28 pipelined steps per thread at 112 x 64 channels (2: 247 us, 4: 238, 8-28: 230)
    if ((int64_t)rpb * w * cv < 2048) rpb = (int)((2048 + (int64_t)w * cv - 1) / ((int64_t)w * cv));
    const int groups = (total_rows + rpb - 1) / rpb;
    return PoolFusedGrid{rpb, groups, pool_fused_remap((unsigned)groups)};
}

}  // namespace iif_plan
