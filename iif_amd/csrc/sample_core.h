// The random sampler (base_sampler.py:35-102 + random_sampler.py:32-82), once: the budget rule, the histogram of the top
// 12 key bits per class and the whole select step, on the packed block scan of block_scan.h.  targets.hip (iif_random_sample)
// and rpn_stage.hip (iif_rpn_stage_targets) run sample_select_core, each through a policy; roi_stage.hip keeps its own
// in-register radix select and takes the budgets from here.  The rule: a class (0 positive, 1 negative) with more members than its budget k
// keeps the k SMALLEST (key, index) pairs - equal keys go to the lower index.
#pragma once
#include "block_scan.h"

namespace {

constexpr int kBins = 4096;                   // top 12 of the 31 key bits
constexpr int kLowBits = 19;
constexpr unsigned kLowMask = (1u << kLowBits) - 1u;

__device__ __forceinline__ unsigned half_of(u64 v, int c) { return c ? (unsigned)(v >> 32) : (unsigned)v; }
__device__ __forceinline__ u64 one_of(int c) { return c ? (1ull << 32) : 1ull; }
__device__ __forceinline__ unsigned sample_key(int32_t k) { return (unsigned)k & 0x7fffffffu; }

// The two budgets from the class totals P (positives) and Q (negatives): base_sampler.py:83-95
struct Budgets { long long kp, kn; };

__device__ __forceinline__ Budgets sample_budgets(long long P, long long Q, int nep, int num, double ub) {
    const long long kp = P < nep ? P : nep;                           // :83-89
    long long budget = num - kp;                                      // :90-95
    if (ub >= 0.0) {
        const double capd = ub * (double)(kp > 1 ? kp : 1);
        if (capd < (double)budget) budget = (long long)capd;          // int(): truncation
    }
    return Budgets{kp, Q < budget ? Q : budget};
}

// The histogram of the top 12 key bits per class, 2 x kBins counters in LDS: clear (the caller synchronises), add, and the
// flush with integer global atomics (after a __syncthreads), by a block of kT threads.
template <int kT>
__device__ __forceinline__ void hist_clear(unsigned* s_hist) {
    for (int i = threadIdx.x; i < 2 * kBins; i += kT) s_hist[i] = 0u;
}
__device__ __forceinline__ void hist_add(unsigned* s_hist, int cls, unsigned key) {
    atomicAdd(&s_hist[cls * kBins + (int)(key >> kLowBits)], 1u);
}
template <int kT>
__device__ __forceinline__ void hist_flush(const unsigned* s_hist, unsigned* hist) {
    for (int i = threadIdx.x; i < 2 * kBins; i += kT)
        if (s_hist[i] != 0u) atomicAdd(hist + i, s_hist[i]);
}

// four consecutive words of the per-candidate array from 4 g on (0 past the end)
__device__ __forceinline__ u32x4 load_words(const unsigned* w, int64_t g, int N) {
    const int64_t i = 4 * g;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (i + 3 < N) return *reinterpret_cast<const u32x4*>(w + i);
    if (i < N) v.x = w[i];
    if (i + 1 < N) v.y = w[i + 1];
    if (i + 2 < N) v.z = w[i + 2];
    return v;
}

// the bin of `h` (this thread's count of bin threadIdx.x, per class) in which the r-th smallest of a class falls, r >= 1
__device__ __forceinline__ void find_bin(u64 mine, u64 ex, const unsigned* r, int* s_bin, unsigned* s_rem) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const unsigned e = half_of(ex, c), h = half_of(mine, c);
        if (r[c] > 0u && e < r[c] && r[c] <= e + h) {
            s_bin[c] = threadIdx.x;
            s_rem[c] = r[c] - e;
        }
    }
}

// What one launch of the select works on: one image's candidates and outputs.  hist: the 2 x kBins counters of the histogram
// pass; ticket: zero on entry; w: one word per candidate (N rounded up to 4 readable); pos_inds [nep], neg_inds [num],
// counts [2].
struct SelectViews {
    int N, nep, num; double ub;
    const unsigned* hist; unsigned* ticket; unsigned* w;
    int64_t* pos_inds; int64_t* neg_inds; int64_t* counts;
};

// The select step, a grid of blocks of kSelThreads per image.  Every block scans the counters: class totals, hence both
// budgets, each class's threshold bin T and the number r it must still take from that bin.  A candidate below T is selected
// outright, one in T is a BOUNDARY candidate; the grid leaves one word per candidate (0 nothing, 1 / 2 selected, 3 + class << 19
// | low 19 key bits: boundary).  The last block to finish (a ticket, no waiting) then works alone on those words: two more digit
// histograms (10 and 9 bits) give each class's threshold KEY and the number to take among the candidates that have exactly that
// key; one ordered sweep (block scans, tile by tile) takes them in index order and writes the index lists - ascending because
// the sweep is - their -1 tails and the counts.  The boundary may be all N candidates: nothing here depends on its length.
//
// The policy P is a SelectViews (public base or members of those names) plus
//   int cls(int64_t i) const        -1 takes no part, 0 positive, 1 negative
//   unsigned key(int64_t i) const   sample_key of the candidate's key
//   static constexpr bool kFlags    true: int8_t* flags gets 0 / 1 / 2 per candidate (all but the boundary candidates in the
//                                   grid-wide pass, those in the sweep)
//   void placed(unsigned slot, int64_t i) const   the sweep put positive i at pos_inds[slot]
//   void padded(int slot) const                   pos_inds[slot] is a -1 tail slot
template <class P>
__device__ __forceinline__ void sample_select_core(const P& p) {
    __shared__ u64 s_scan[kSelThreads / 64 + 1];
    __shared__ unsigned s_h[2 * 1024];
    __shared__ int s_T[2], s_T2[2], s_T3[2];
    __shared__ unsigned s_r[2], s_r2[2], s_r3[2];
    __shared__ bool s_last;
    const int tid = threadIdx.x;
    const int N = p.N;

    // ---- class totals, budgets, threshold bins: every block for itself (thread t owns bins 4 t .. 4 t + 3 of both classes)
    const u32x4 h0 = reinterpret_cast<const u32x4*>(p.hist)[tid];
    const u32x4 h1 = reinterpret_cast<const u32x4*>(p.hist + kBins)[tid];
    const unsigned c0 = h0.x + h0.y + h0.z + h0.w, c1 = h1.x + h1.y + h1.z + h1.w;
    u64 total;
    const u64 ex = block_scan_excl((u64)c0 | ((u64)c1 << 32), s_scan, &total);
    const long long M[2] = {(unsigned)total, (unsigned)(total >> 32)};
    const Budgets bu = sample_budgets(M[0], M[1], p.nep, p.num, p.ub);
    const int kp = __builtin_amdgcn_readfirstlane((int)bu.kp);         // the same in every lane, and 0 <= k <= num < 2^31:
    const int kn = __builtin_amdgcn_readfirstlane((int)bu.kn);         // one scalar register each through the sweep
    const long long k[2] = {kp, kn};
    if (tid < 2) {
        s_T[tid] = k[tid] <= 0 ? -1 : kBins;                           // nothing / everything of the class, unless found below
        s_r[tid] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (k[c] > 0 && k[c] < M[c]) {
            const u32x4 hh = c ? h1 : h0;
            const unsigned hv[4] = {hh.x, hh.y, hh.z, hh.w};
            long long cum = half_of(ex, c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (cum < k[c] && k[c] <= cum + hv[j]) {
                    s_T[c] = 4 * tid + j;
                    s_r[c] = (unsigned)(k[c] - cum);
                }
                cum += hv[j];
            }
        }
    }
    __syncthreads();
    const int T[2] = {s_T[0], s_T[1]};
    const unsigned r[2] = {s_r[0], s_r[1]};

    // ---- the grid-wide pass: one word per candidate, the flags of all but the boundary candidates
    const int64_t step = (int64_t)gridDim.x * kSelThreads;
    for (int64_t i = (int64_t)blockIdx.x * kSelThreads + tid; i < N; i += step) {
        const int cls = p.cls(i);
        unsigned ww = 0u;
        bool boundary = false;
        if (cls >= 0) {
            const unsigned key = p.key(i);
            const int bin = (int)(key >> kLowBits);
            if (bin < T[cls]) ww = 1u + cls;
            else if (bin == T[cls]) { ww = 3u + (((unsigned)cls << kLowBits) | (key & kLowMask)); boundary = true; }
        }
        p.w[i] = ww;
        if constexpr (P::kFlags) { if (!boundary) p.flags[i] = (int8_t)ww; }
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();

    // ---- the last block, alone: the threshold key of each class among its boundary candidates, low 19 bits in two digits
    const int64_t groups = ((int64_t)N + 3) / 4;
    if (tid < 2) { s_T2[tid] = 0; s_T3[tid] = 0; s_r2[tid] = 0u; s_r3[tid] = 0u; }
    s_h[tid] = 0u;
    s_h[1024 + tid] = 0u;
    __syncthreads();
    if (r[0] > 0u || r[1] > 0u) {
        for (int64_t g = tid; g < groups; g += kSelThreads) {
            const u32x4 v = load_words(p.w, g, N);
            const unsigned e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e4[j] >= 3u) {
                    const unsigned e = e4[j] - 3u;
                    atomicAdd(&s_h[(e >> kLowBits) * 1024u + ((e & kLowMask) >> 9)], 1u);
                }
        }
        __syncthreads();
        const u64 mine = (u64)s_h[tid] | ((u64)s_h[1024 + tid] << 32);
        u64 tot;
        const u64 ex2 = block_scan_excl(mine, s_scan, &tot);
        find_bin(mine, ex2, r, s_T2, s_r2);
        __syncthreads();
        const int T2[2] = {s_T2[0], s_T2[1]};
        const unsigned r2[2] = {s_r2[0], s_r2[1]};
        s_h[tid] = 0u;
        __syncthreads();
        for (int64_t g = tid; g < groups; g += kSelThreads) {
            const u32x4 v = load_words(p.w, g, N);
            const unsigned e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e4[j] >= 3u) {
                    const unsigned e = e4[j] - 3u;
                    const unsigned cls = e >> kLowBits, low = e & kLowMask;
                    if ((int)(low >> 9) == T2[cls]) atomicAdd(&s_h[cls * 512u + (low & 511u)], 1u);
                }
        }
        __syncthreads();
        const u64 mine3 = tid < 512 ? ((u64)s_h[tid] | ((u64)s_h[512 + tid] << 32)) : 0ull;
        const u64 ex3 = block_scan_excl(mine3, s_scan, &tot);
        find_bin(mine3, ex3, r2, s_T3, s_r3);
        __syncthreads();
    }
    unsigned K[2], r3[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        K[c] = ((unsigned)s_T2[c] << 9) | (unsigned)s_T3[c];
        r3[c] = s_r3[c];
    }

    // ---- the ordered sweep: tile by tile in index order; among the candidates with exactly the threshold key the first r3
    u64 run_eq = 0ull, run_sel = 0ull;
    const int64_t tiles = (groups + kSelThreads - 1) / kSelThreads;
    for (int64_t t = 0; t < tiles; ++t) {
        const int64_t g = t * kSelThreads + tid;
        const u32x4 v = load_words(p.w, g, N);
        const unsigned e4[4] = {v.x, v.y, v.z, v.w};
        int cls4[4], kind4[4];                                         // kind: 0 not selected, 1 selected, 2 has the threshold key
        u64 eq = 0ull;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cls4[j] = 0; kind4[j] = 0;
            if (e4[j] == 1u || e4[j] == 2u) { cls4[j] = (int)e4[j] - 1; kind4[j] = 1; }
            else if (e4[j] >= 3u) {
                const unsigned e = e4[j] - 3u;
                const unsigned low = e & kLowMask;
                cls4[j] = (int)(e >> kLowBits);
                if (low < K[cls4[j]]) kind4[j] = 1;
                else if (low == K[cls4[j]]) { kind4[j] = 2; eq += one_of(cls4[j]); }
            }
        }
        u64 tot;
        u64 rank = block_scan_excl(eq, s_scan, &tot) + run_eq;
        run_eq += tot;
        u64 sel = 0ull;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (kind4[j] == 2) {
                kind4[j] = half_of(rank, cls4[j]) < r3[cls4[j]] ? 1 : 0;
                rank += one_of(cls4[j]);
            }
            if (kind4[j] == 1) sel += one_of(cls4[j]);
        }
        u64 at = block_scan_excl(sel, s_scan, &tot) + run_sel;
        run_sel += tot;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t idx = 4 * g + j;
            if constexpr (P::kFlags) { if (e4[j] >= 3u) p.flags[idx] = (int8_t)(kind4[j] == 1 ? 1 + cls4[j] : 0); }
            if (kind4[j] != 1) continue;
            const unsigned slot = half_of(at, cls4[j]);
            at += one_of(cls4[j]);
            if (slot >= (unsigned)(cls4[j] ? kn : kp)) continue;       // cannot happen: the select takes exactly k
            if (cls4[j] == 1) { p.neg_inds[slot] = idx; continue; }
            p.pos_inds[slot] = idx;
            p.placed(slot, idx);
        }
    }
    for (int j = kp + tid; j < p.nep; j += kSelThreads) {
        p.pos_inds[j] = -1;
        p.padded(j);
    }
    for (int j = kn + tid; j < p.num; j += kSelThreads) p.neg_inds[j] = -1;
    if (tid == 0) {
        p.counts[0] = kp;
        p.counts[1] = kn;
    }
}

}  // namespace
