// What the NMS files share (nms.hip, multiclass_nms.hip); every piece exists here and nowhere else.
//   keys      fkey / fkey_inv: the order-preserving bits of a float.  sort_key: valid << 56 | score bits << 24 | ~index, so a
//             greater key is a higher score, equal scores go to the lower index and boxes that take no part come last;
//             key_index / key_valid take it apart.  box_max_key: a box's largest coordinate as such bits, for integer maxima.
//   overlap   nms_area, nms_intersection and the two forms of mmcv's test: nms_suppresses, and nms_suppresses_quick, which
//             leaves the quotient out where it cannot decide.  Single float32 operations in mmcv's order (-ffp-contract=off).
//   rank      count_greater_tiled: "how many keys are greater than mine", the keys streamed through an LDS tile;
//             count_greater_lds: the same over keys that already lie in LDS, for P keys per thread in one sweep.
//   resolve   resolve_block64: the greedy walk over one block of 64 ranks in one wave, and the trim to the room under the cap.
//   select    select_pass_core: one launch of the six-launch radix select of the k largest 56-bit numbers of a segment, in digits
//             of 12, 12, 12, 12 and 8 bits.  The numbers of a segment are distinct, so five digits give the exact threshold.
#pragma once
#include "block_scan.h"

constexpr int kSelBlocks = 16;                // blocks per segment in a selection pass; thread t owns bins 4 t .. 4 t + 3
constexpr int kBins = 4096;
constexpr int kPasses = 5;                    // digits of 12, 12, 12, 12, 8 bits
constexpr int kRankTile = 1024;
constexpr u32 kIndexMask = 0xFFFFFFu;

struct SelState { u64 prefix; u32 rem; u32 pad; };

// bits that order as unsigned integers the way the floats order; -0 and +0 are one value
__device__ __forceinline__ u32 fkey(float f) {
    u32 u = __float_as_uint(f);
    if (f == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(u32 k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ __forceinline__ u64 sort_key(u32 score_bits, int index, bool valid = false) {
    return ((u64)(valid ? 1u : 0u) << 56) | ((u64)score_bits << 24) | (u64)(kIndexMask - (u32)index);
}
__device__ __forceinline__ int key_index(u64 key) { return (int)(kIndexMask - ((u32)key & kIndexMask)); }
__device__ __forceinline__ bool key_valid(u64 key) { return (key >> 56) & 1ull; }
__device__ __forceinline__ u32 box_max_key(float x1, float y1, float x2, float y2) { return fkey(fmaxf(fmaxf(x1, y1), fmaxf(x2, y2))); }

__device__ __forceinline__ u32 wave_max_u(u32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u32 t = (u32)__shfl_xor((int)v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// a padding row of dets [.., 5]
__device__ __forceinline__ void zero_det_row(float* d) { d[0] = 0.0f; d[1] = 0.0f; d[2] = 0.0f; d[3] = 0.0f; d[4] = 0.0f; }

// mmcv nms_cuda_kernel.cuh: S = (x2 - x1 + offset) * (y2 - y1 + offset); p suppresses q (or q p: every step is symmetric) when
// inter / (Sp + Sq - inter) > thr.  Single float32 operations in mmcv's order (-ffp-contract=off); a NaN quotient does not suppress.
__device__ __forceinline__ float nms_area(const f32x4 p, float off) { return (p.z - p.x + off) * (p.w - p.y + off); }
__device__ __forceinline__ float nms_intersection(const f32x4 p, const f32x4 q, float off) {
    const float left = fmaxf(p.x, q.x), right = fminf(p.z, q.z);
    const float top = fmaxf(p.y, q.y), bottom = fminf(p.w, q.w);
    const float w = fmaxf(right - left + off, 0.0f), h = fmaxf(bottom - top + off, 0.0f);
    return w * h;
}
__device__ __forceinline__ bool nms_over(float inter, float sp, float sq, float thr) { return inter / (sp + sq - inter) > thr; }
__device__ __forceinline__ bool nms_suppresses(const f32x4 p, float sp, const f32x4 q, float sq, float off, float thr) {
    return nms_over(nms_intersection(p, q, off), sp, sq, thr);
}
// The same result, bit for bit, with q's area and the quotient left out where they cannot decide: inter is >= 0 or NaN, and with
// inter == 0 (or NaN) the quotient is 0, -0 or NaN, none of them above a threshold >= 0.  Most pairs of a walk do not meet.
__device__ __forceinline__ bool nms_suppresses_quick(const f32x4 p, float sp, const f32x4 q, float off, float thr) {
    const float inter = nms_intersection(p, q, off);
    if (thr >= 0.0f && !(inter > 0.0f)) return false;
    return nms_over(inter, sp, nms_area(q, off), thr);
}

// How many of keys[0 .. n) are greater than `my`, for every thread of a block of kT threads at once (all of them call): the keys
// stream through s_tile [kRankTile], four comparisons at a time.
template <int kT>
__device__ __forceinline__ int count_greater_tiled(const u64* keys, int n, u64 my, u64* s_tile) {
    const int tid = threadIdx.x;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += kRankTile) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kRankTile / kT; ++q) {
            const int j = j0 + q * kT + tid;
            s_tile[q * kT + tid] = j < n ? keys[j] : 0ull;                     // 0 is greater than no key
        }
        __syncthreads();
        const int cn = min(kRankTile, (n - j0 + 3) & ~3);
        for (int j = 0; j < cn; j += 4) rank += (s_tile[j] > my) + (s_tile[j + 1] > my) + (s_tile[j + 2] > my) + (s_tile[j + 3] > my);
    }
    return rank;
}

// ... and with the n keys in LDS already: one sweep ranks all P keys of a thread
template <int P>
__device__ __forceinline__ void count_greater_lds(const u64* s_keys, int n, const u64 (&my)[P], int (&rank)[P]) {
#pragma unroll
    for (int k = 0; k < P; ++k) rank[k] = 0;
    for (int j = 0; j < n; ++j) {
        const u64 o = s_keys[j];
#pragma unroll
        for (int k = 0; k < P; ++k) rank[k] += o > my[k];
    }
}

// mmcv's greedy walk over one block of 64 ranks, in one wave from registers (v_readlane).  Lane i holds `diag`, the ranks of the
// block that rank i suppresses (bits above i); `rem` has the ranks that are out already.  Returns the ranks kept, the last ones
// dropped until at most `room` remain.  room is an int: it is cap - total with 0 <= total <= cap, and the cap of either caller is
// an int argument or at most N <= IIF_NMS_MAX_BOXES.
__device__ __forceinline__ u64 resolve_block64(u64 diag, u64 rem, int room) {
    const u32 dlo = (u32)diag, dhi = (u32)(diag >> 32);
    u64 kept = 0ull;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const u64 di = (u64)(u32)__builtin_amdgcn_readlane((int)dlo, i) | ((u64)(u32)__builtin_amdgcn_readlane((int)dhi, i) << 32);
        const bool k = !((rem >> i) & 1ull);
        kept |= k ? (1ull << i) : 0ull;
        rem |= k ? di : 0ull;
    }
    while (__popcll(kept) > room) kept &= ~(1ull << (63 - __clzll((long long)kept)));
    return kept;
}

__device__ __forceinline__ int digit_shift(int p) { return p < 4 ? 44 - 12 * p : 0; }
__device__ __forceinline__ int digit_bits(int p) { return p < 4 ? 12 : 8; }

// One launch `pass` of the select, by a grid of kSelBlocks blocks of kSelThreads per segment.  Pass 0 .. 4 histograms digit
// `pass` among the elements that match the digits found so far (LDS atomics, flushed with integer global atomics); every pass
// >= 1 first turns the histogram of the pass before into the threshold digit (every block for itself; block 0 of the segment
// leaves the state for the next launch); pass 5 takes the elements at or above the threshold.  The policy P has
//   int seg                     the segment's index into hist [.][kPasses][kBins] (zero on entry) and state [.][kPasses]
//   int n, k                    elements of the segment, and how many to take
//   u32* hist; SelState* state
//   bool all                    take every element, without a threshold (the histogram passes need not have run)
//   Item load(int i) const      element i: Item::number is its 56-bit number, the rest is what take reuses
//   void take(int i, const Item&)      pass 5: the element is selected
//   void finish()               pass 5: after the block's last take
// Keep seg, n, k and all uniform over the block (scalar registers).
template <class P>
__device__ __forceinline__ void select_pass_core(P& p, int pass) {
    __shared__ u32 s_h[kBins];
    __shared__ u32 s_scan[kSelThreads / 64 + 1];
    __shared__ u32 s_bin, s_rem;
    const int tid = threadIdx.x;
    SelState st;
    st.prefix = 0ull; st.rem = (u32)p.k; st.pad = 0u;
    if (!p.all && pass >= 1) {
        if (pass >= 2) st = p.state[p.seg * kPasses + pass - 2];
        const u32x4 h = reinterpret_cast<const u32x4*>(p.hist + ((int64_t)p.seg * kPasses + pass - 1) * kBins)[tid];
        const u32 hv[4] = {h.x, h.y, h.z, h.w};
        if (tid == 0) { s_bin = 0u; s_rem = 1u; }
        u32 cum = block_scan_excl(h.x + h.y + h.z + h.w, s_scan);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (cum < st.rem && st.rem <= cum + hv[j]) { s_bin = 4u * tid + j; s_rem = st.rem - cum; }
            cum += hv[j];
        }
        __syncthreads();
        const int bits = digit_bits(pass - 1);
        st.prefix = (st.prefix << bits) | (u64)(((1u << bits) - 1u) - s_bin);      // bins run from the largest digit down
        st.rem = s_rem;
        if (blockIdx.x == 0 && tid == 0) p.state[p.seg * kPasses + pass - 1] = st;
    }
    const bool gather = pass == kPasses;
    if (!gather) {
        for (int i = tid; i < kBins; i += kSelThreads) s_h[i] = 0u;
        __syncthreads();
    }
    const int shift = gather ? 0 : digit_shift(pass);
    const u32 dmask = gather ? 0u : (1u << digit_bits(pass)) - 1u;
    const int pshift = pass >= 1 ? digit_shift(pass - 1) : 0;
    for (int base = blockIdx.x * kSelThreads; base < p.n; base += kSelBlocks * kSelThreads) {     // a uniform trip count
        const int i = base + tid;
        if (i >= p.n) continue;
        const auto it = p.load(i);
        if (!gather) {
            if (pass == 0 || (it.number >> pshift) == st.prefix) atomicAdd(&s_h[dmask - ((u32)(it.number >> shift) & dmask)], 1u);
        } else if (p.all || it.number >= st.prefix) {
            p.take(i, it);
        }
    }
    if (gather) {
        p.finish();
    } else {
        __syncthreads();
        u32* hist = p.hist + ((int64_t)p.seg * kPasses + pass) * kBins;
        for (int i = tid; i < kBins; i += kSelThreads)
            if (s_h[i] != 0u) atomicAdd(hist + i, s_h[i]);
    }
}
