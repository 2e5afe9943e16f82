// The scalar-loss reduction shared by the fused loss heads (iif_head.hip, sigmoid_head.hip, bce_head.hip, bbox_reg_head.hip,
// seesaw_head.hip): K sums leave the launch that produced them, deterministically, without a second launch; and the one-block
// reduce kernel for the launches that have no workspace (iif_head.hip, sigmoid_head.hip, mask_head.hip).
#pragma once
#include "common.h"

namespace {

// Partial slots of the single-launch loss workspace (IIF_CE_WORKSPACE_BYTES = one int32 ticket + one float per block):
// a launch that passes that workspace to ticketed_finish runs at most this many blocks.
constexpr unsigned kCePartialSlots = IIF_CE_WORKSPACE_BYTES / 4 - 1;
static_assert(IIF_CE_WORKSPACE_BYTES == 4 * (1 + kCePartialSlots), "the CE workspace is a ticket word and whole float slots");

// Called by every thread of every block at the end of a kernel of at most 256 threads (a power of two of waves), with each
// wave's K sums in `wave` (wave-uniform).  out[k] = scale[k] * (sum over all waves of the grid of wave[k]).
//
// ticket: an int32 that is zero on entry and zero again on exit.  A head whose caller may ask for no scalar passes a null ticket
// and tests it, block-uniformly, around this call; the test is not in here because the Seesaw kernel always has a workspace.
// The partials are K * gridDim.x floats that start `partial_word` 32-bit words behind the ticket, the K sums of a block side by
// side (the default is the CE workspace: the ticket word, then one float per block).
//
// Order of the additions, fixed for a given grid: thread 0 of a block adds its waves in index order and publishes the block's
// partial; the last block to take a ticket has thread t add the partials of blocks t, t + blockDim.x, ... and then a halving
// tree over blockDim.x folds the threads.  No float atomics: bit-identical from call to call.
//
// There is deliberately NO release fence before the ticket.  An agent-scope fence writes back the whole XCD L2, which at this
// point is full of the gradient rows just stored (it cost 40 % of the CE kernel).  Instead the partial goes out as an
// agent-scope atomic exchange - performed at the coherence point, and a returning atomic has completed when its value is
// back; the s_waitcnt vmcnt(0) takes the returned value(s) as operands so that it cannot move above them - the ticket is taken
// only after that, and the last block reads the partials with agent-scope atomic loads: the same ordering without touching the
// ordinary stores.  The re-zeroing store makes the workspace reusable by the next launch on the stream, of any head.
template <int K>
__device__ __forceinline__ void ticketed_finish(int32_t* ticket, const float (&wave)[K], const float (&scale)[K],
                                                float* const (&out)[K], int partial_word = 1) {
    static_assert(K == 1 || K == 2, "one s_waitcnt operand list per K");
    __shared__ float sh[K][256];
    __shared__ int last;
    float* partial = reinterpret_cast<float*>(ticket + partial_word);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sh[k][w] = wave[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc[K], prev[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.f;
        for (int i = 0; i < wpb; ++i) {
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += sh[k][i];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            prev[k] = __hip_atomic_exchange(partial + K * blockIdx.x + k, acc[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (K == 1) asm volatile("s_waitcnt vmcnt(0)" : : "v"(prev[0]) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" : : "v"(prev[0]), "v"(prev[1]) : "memory");
        const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (t == (int)gridDim.x - 1);
    }
    __syncthreads();
    if (!last) return;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += __hip_atomic_load(partial + K * i + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) *out[k] = sh[k][0] * scale[k];
        __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The launch without a workspace: *out = scale * (fixed-order sum of rows[0 .. n)) accumulated in A (float, or double for the
// mask loss), one 256-thread block, deterministic.
template <typename A>
__global__ void __launch_bounds__(256) rows_reduce_kernel(const float* rows, int n, A scale, float* out) {
    __shared__ A sh[256];
    A acc = 0;
    for (int i = threadIdx.x; i < n; i += 256) acc += (A)rows[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = (float)(sh[0] * scale);
}

}  // namespace
