// The scalar-loss reduction shared by the fused loss heads (iif_head.hip, sigmoid_head.hip, bce_head.hip, bbox_reg_head.hip,
// seesaw_head.hip, head_loss.hip): a few float sums, and the integer counts that go with them, leave the launch that produced
// them, deterministically, without a second launch; and the one-block reduce kernel for the launches that have no workspace
// (iif_head.hip, sigmoid_head.hip, mask_head.hip).
#pragma once
#include "common.h"

namespace {

// Partial slots of the single-launch loss workspace (IIF_CE_WORKSPACE_BYTES = one int32 ticket + one float per block):
// a launch that passes that workspace to ticketed_finish runs at most this many blocks.
constexpr unsigned kCePartialSlots = IIF_CE_WORKSPACE_BYTES / 4 - 1;
static_assert(IIF_CE_WORKSPACE_BYTES == 4 * (1 + kCePartialSlots), "the CE workspace is a ticket word and whole float slots");

// blockDim.x as the scalar load it is for HIP's whole blocks.  blockDim.x itself first asks whether this is a partial last block
// and then reads its answer with a VECTOR load; at the end of a kernel the wait for that load also waits for the gradient rows
// just stored, before the partials can even go out (0.4 us of an 11 us head kernel).  A kernel that also reads it before its row
// loop (for its waves per block) has the value in a register when the reduction asks for it.
__device__ __forceinline__ int block_threads() { return __builtin_amdgcn_workgroup_size_x(); }

// The core.  Called by every thread of every block at the end of a kernel of at most 256 threads (a power of two of waves), with
// each wave's NF float and NI integer sums in f and n (wave-uniform; NI == 0: n is one unused element).  True in thread 0 of the
// last block only, which then holds the sums over all waves of the grid in f and n, has to write its results and has to put the
// ticket back to zero; the heads turn the totals into different outputs, so neither is done here.
//
// The block's threads are read from the launch (block_threads()) unless the kernel names the one size it is launched with as
// NT: with every trip count a constant the end of the kernel is 0.15 us shorter (measured on all nine entries), which is what
// the read-free BBoxHead.loss kernels had before they shared this code.
//
// ticket: an int32 that is zero on entry.  partial: (NF + NI) * gridDim.x 32-bit words, the sums of a block side by side, floats
// first; nothing in them has to be zero - a block's words are overwritten before the ticket that lets them be read.
//
// Order of the additions, fixed for a given grid: thread 0 of a block adds its waves in index order and publishes the block's
// partial; the last block to take a ticket has thread t add the partials of blocks t, t + blockDim.x, ... and then a halving
// tree over blockDim.x folds the threads.  Integers are added as integers, and there are no float atomics: bit-identical from
// call to call.
//
// There is deliberately NO release fence before the ticket.  An agent-scope fence writes back the whole XCD L2, which at this
// point is full of the gradient rows just stored (it cost 40 % of the CE kernel).  Instead the partial, float or integer, goes
// out as an agent-scope atomic exchange - performed at the coherence point, and a returning atomic has completed when its value
// is back; the s_waitcnt vmcnt(0) takes one operand that depends on every returned value (their bit patterns OR-ed) so that it
// cannot move above them - the ticket is taken only after that, and the last block reads the partials with agent-scope atomic
// loads: the same ordering without touching the ordinary stores.  The caller's re-zeroing store makes the workspace reusable by
// the next launch on the stream, of any head.
template <int NF, int NI, int NT = 0>
__device__ __forceinline__ bool ticketed_sums(int32_t* ticket, int32_t* partial, float (&f)[NF], int (&n)[NI > 0 ? NI : 1]) {
    static_assert(NF >= 1 && NI >= 0, "at least the loss itself");
    __shared__ float sh_f[NF][256];
    __shared__ int sh_n[NI > 0 ? NI : 1][256];
    __shared__ int last;
    const int nt = NT ? NT : block_threads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = nt >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NF; ++k) sh_f[k][w] = f[k];
#pragma unroll
        for (int k = 0; k < NI; ++k) sh_n[k][w] = n[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NF; ++k) f[k] = 0.f;
#pragma unroll
        for (int k = 0; k < NI; ++k) n[k] = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {              // all four waves' slots are read at once; a wave that is not there adds nothing
#pragma unroll
            for (int k = 0; k < NF; ++k) f[k] = i < wpb ? f[k] + sh_f[k][i] : f[k];
#pragma unroll
            for (int k = 0; k < NI; ++k) n[k] = i < wpb ? n[k] + sh_n[k][i] : n[k];
        }
        int32_t* mine = partial + (NF + NI) * blockIdx.x;
        unsigned keep = 0;
#pragma unroll
        for (int k = 0; k < NF; ++k)
            keep |= __float_as_uint(__hip_atomic_exchange(reinterpret_cast<float*>(mine + k), f[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
        for (int k = 0; k < NI; ++k) keep |= (unsigned)__hip_atomic_exchange(mine + NF + k, n[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" : : "v"(keep) : "memory");
        const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (t == (int)gridDim.x - 1);
    }
    __syncthreads();
    if (!last) return false;
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = 0.f;
#pragma unroll
    for (int k = 0; k < NI; ++k) n[k] = 0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += nt) {
        const int32_t* theirs = partial + (NF + NI) * i;
#pragma unroll
        for (int k = 0; k < NF; ++k)
            f[k] += __hip_atomic_load(reinterpret_cast<const float*>(theirs + k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < NI; ++k) n[k] += __hip_atomic_load(theirs + NF + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NF; ++k) sh_f[k][threadIdx.x] = f[k];
#pragma unroll
    for (int k = 0; k < NI; ++k) sh_n[k][threadIdx.x] = n[k];
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {            // the steps o < blockDim.x of them (block-uniform), at constant offsets
        if (__builtin_expect(o >= nt, 0)) continue;        // (expected to run: keeps the steps in line, not behind the kernel's end)
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < NF; ++k) sh_f[k][threadIdx.x] += sh_f[k][threadIdx.x + o];
#pragma unroll
            for (int k = 0; k < NI; ++k) sh_n[k][threadIdx.x] += sh_n[k][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = sh_f[k][0];
#pragma unroll
    for (int k = 0; k < NI; ++k) n[k] = sh_n[k][0];
    return true;
}

// The float-only form: out[k] = scale[k] * (sum over all waves of the grid of wave[k]), and the ticket is zero again on exit.
// A head whose caller may ask for no scalar passes a null ticket and tests it, block-uniformly, around this call; the test is
// not in here because the Seesaw kernel always has a workspace.  The partials start `partial_word` 32-bit words behind the
// ticket (the default is the CE workspace: the ticket word, then one float per block).
template <int K>
__device__ __forceinline__ void ticketed_finish(int32_t* ticket, const float (&wave)[K], const float (&scale)[K],
                                                float* const (&out)[K], int partial_word = 1) {
    float f[K];
    int none[1];
#pragma unroll
    for (int k = 0; k < K; ++k) f[k] = wave[k];
    if (!ticketed_sums<K, 0>(ticket, ticket + partial_word, f, none)) return;
#pragma unroll
    for (int k = 0; k < K; ++k) *out[k] = f[k] * scale[k];
    __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
