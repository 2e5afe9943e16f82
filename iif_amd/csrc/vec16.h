// Element I/O of the kernels templated on the storage type T: float, or unsigned short holding bf16 bits.  T in memory, fp32 in
// registers; this is the only place that knows how T is laid out.
//   VT<T>        one element (load1 / store1), a group of four (load4 / store4: 16 B fp32, 8 B bf16) and the 16-byte vector of
//                V = 4 fp32 / 8 bf16 elements: converted at once (load / store), held raw and unpacked later (raw / unpack), with
//                a non-temporal hint (_nt, store_as) or as the 8-byte-aligned vector of a row that may end on a half (raw_row ...)
//   VTn<T, V>    the same under one name for a body compiled at V = 1, V = 4 and V = VT<T>::V
//   load_f32<V> / store_f32<V>   contiguous fp32 side arrays of such a body
#pragma once
#include "common.h"

namespace {
template <typename T> struct VT;
template <> struct VT<float> {
    static constexpr int V = 4;
    using Raw = u32x4;
    static __device__ __forceinline__ float load1(const float* p) { return *p; }
    static __device__ __forceinline__ void store1(float* p, float v) { *p = v; }
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
        *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    }
    static __device__ __forceinline__ void load4(const float* p, float (&v)[4]) { load(p, v); }
    static __device__ __forceinline__ void store4(float* p, const float (&v)[4]) { store(p, v); }
    // Non-temporal load: the line will not be used again for a long time (an activation that is next read in backward, an
    // operand at its last use).  The hint keeps it from displacing what the NEXT kernel reads back (the tensor this kernel
    // writes) in L2 / the Infinity Cache: -2.2 % on the ResNet50 step from the two BN apply kernels alone.
    static __device__ __forceinline__ void load_nt(const float* p, float (&v)[4]) {
        const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    // The 16 raw bytes first, the conversion later: a batch of loads can be requested before the first value is touched, and
    // rows in flight cost 4 registers per lane and vector whatever the element type.  (bf16 rows are half the bytes, so a wave
    // keeps two of them in flight to give a CU the bytes of one fp32 row: with one, the classifier head ran [65536, 1000] bf16
    // at 3.2 TB/s against 4.9 for fp32.)
    static __device__ __forceinline__ Raw raw_nt(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }
    static __device__ __forceinline__ Raw raw(const float* p) { return *reinterpret_cast<const u32x4*>(p); }
    static __device__ __forceinline__ void unpack(const Raw& t, float (&v)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(t[i]);
    }
    // The same 16 bytes typed as the floats they are.  The fp32 kernels of bce_head.hip and iif_head.hip compile to other code
    // from the two types (bce_det_kernel: another register allocation) and stay on the one they were tuned and measured with.
    using RawF = f32x4;
    static __device__ __forceinline__ RawF rawf(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
    static __device__ __forceinline__ void unpack(const RawF& t, float (&v)[4]) { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    static __device__ __forceinline__ float dword_elem(unsigned w, int) { return __uint_as_float(w); }      // element e of a raw dword
    static __device__ __forceinline__ float round_trip(float v) { return v; }       // a value as the storage type holds it
    template <bool NT> static __device__ __forceinline__ void store_as(float* p, const float (&v)[4]) {
        const f32x4 t{v[0], v[1], v[2], v[3]};
        if (NT) __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(p)); else *reinterpret_cast<f32x4*>(p) = t;
    }
    // the row forms of the bf16 specialisation; an fp32 vector is whole or absent
    static __device__ __forceinline__ Raw raw_row(const float* p, int nv) { return nv > 0 ? raw(p) : u32x4{0u, 0u, 0u, 0u}; }
    static __device__ __forceinline__ RawF raw_row_some(const float* p, int) { return rawf(p); }
    static __device__ __forceinline__ void store_row_some(float* p, int, const float (&v)[4]) { store(p, v); }
};
template <> struct VT<unsigned short> {
    static constexpr int V = 8;
    using Raw = u32x4;
    using RawF = Raw;
    static __device__ __forceinline__ float load1(const unsigned short* p) { return bf16_bits_to_f32(*p); }
    static __device__ __forceinline__ void store1(unsigned short* p, float v) { *p = f32_to_bf16_bits(v); }
    static __device__ __forceinline__ Raw raw_nt(const unsigned short* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }
    static __device__ __forceinline__ Raw raw(const unsigned short* p) { return *reinterpret_cast<const u32x4*>(p); }
    static __device__ __forceinline__ void unpack(const Raw& t, float (&v)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = bf16_bits_to_f32(t[i] & 0xffffu); v[2 * i + 1] = __uint_as_float(t[i] & 0xffff0000u); }
    }
    static __device__ __forceinline__ float dword_elem(unsigned w, int e) {
        return (e & 1) ? __uint_as_float(w & 0xffff0000u) : bf16_bits_to_f32(w & 0xffffu);
    }
    static __device__ __forceinline__ Raw pack(const float (&v)[8]) {
        u32x4 t;
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
        return t;
    }
    static __device__ __forceinline__ void load(const unsigned short* p, float (&v)[8]) { unpack(raw(p), v); }
    static __device__ __forceinline__ void load_nt(const unsigned short* p, float (&v)[8]) { unpack(raw_nt(p), v); }
    static __device__ __forceinline__ void store(unsigned short* p, const float (&v)[8]) { *reinterpret_cast<u32x4*>(p) = pack(v); }
    static __device__ __forceinline__ void load4(const unsigned short* p, float (&v)[4]) {
        const u32x2 t = *reinterpret_cast<const u32x2*>(p);
#pragma unroll
        for (int i = 0; i < 2; ++i) { v[2 * i] = bf16_bits_to_f32(t[i] & 0xffffu); v[2 * i + 1] = __uint_as_float(t[i] & 0xffff0000u); }
    }
    static __device__ __forceinline__ u32x2 pack4(const float (&v)[4]) { return u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])}; }
    static __device__ __forceinline__ void store4(unsigned short* p, const float (&v)[4]) { *reinterpret_cast<u32x2*>(p) = pack4(v); }
    static __device__ __forceinline__ float round_trip(float v) { return bf16_bits_to_f32(f32_to_bf16_bits(v)); }
    template <bool NT> static __device__ __forceinline__ void store_as(unsigned short* p, const float (&v)[8]) {
        if (NT) __builtin_nontemporal_store(pack(v), reinterpret_cast<u32x4*>(p)); else *reinterpret_cast<u32x4*>(p) = pack(v);
    }
    // 8-byte aligned 16-byte vectors: the rows of a CONTIGUOUS [B, C] matrix with C % 8 == 4 (LVIS: 1204) start on alternate
    // 8-byte boundaries; gfx950 runs with unaligned access enabled, so the access stays one dwordx4 (such a matrix used to fall
    // back to a streaming kernel).  nv = the columns of the vector that exist: 8, or 4 for the 8-byte half that ends such a row.
    typedef u32x4 u32x4_a8 __attribute__((aligned(8)));
    // raw_row: nv in {0, 4, 8}, nothing is read and zeros come back for 0 (eval_stats.hip: a lane beyond the row's end calls it too)
    static __device__ __forceinline__ Raw raw_row(const unsigned short* p, int nv) {
        u32x4 w = u32x4{0u, 0u, 0u, 0u};
        if (nv == 8) w = *reinterpret_cast<const u32x4_a8*>(p);
        else if (nv == 4) { const u32x2 h = *reinterpret_cast<const u32x2*>(p); w.x = h.x; w.y = h.y; }
        return w;
    }
    // raw_row_some / store_row_some: nv in {4, 8} only, one test less (iif_head.hip: its lanes without columns do not call)
    static __device__ __forceinline__ RawF raw_row_some(const unsigned short* p, int nv) {
        u32x4 w = u32x4{0u, 0u, 0u, 0u};
        if (nv == 8) w = *reinterpret_cast<const u32x4_a8*>(p);
        else { const u32x2 h = *reinterpret_cast<const u32x2*>(p); w.x = h.x; w.y = h.y; }
        return w;
    }
    static __device__ __forceinline__ void store_row_some(unsigned short* p, int nv, const float (&v)[8]) {
        const u32x4 w = pack(v);
        if (nv == 8) *reinterpret_cast<u32x4_a8*>(p) = w;
        else *reinterpret_cast<u32x2*>(p) = u32x2{w.x, w.y};
    }
};

// V elements under one name: V = 1 is the scalar form, 4 the group of four, VT<T>::V the 16-byte vector (raw / unpack included)
template <typename T, int V> struct VTn;
template <typename T> struct VTn<T, 1> {
    using Raw = T;
    static __device__ __forceinline__ Raw raw(const T* p) { return *p; }
    static __device__ __forceinline__ void unpack(const Raw& t, float (&v)[1]) { v[0] = VT<T>::load1(&t); }
    static __device__ __forceinline__ void load(const T* p, float (&v)[1]) { v[0] = VT<T>::load1(p); }
    static __device__ __forceinline__ void store(T* p, const float (&v)[1]) { VT<T>::store1(p, v[0]); }
};
template <> struct VTn<float, 4> : VT<float> {
    using Raw = RawF;
    static __device__ __forceinline__ Raw raw(const float* p) { return rawf(p); }
};
template <> struct VTn<unsigned short, 8> : VT<unsigned short> {};
template <> struct VTn<unsigned short, 4> {
    static __device__ __forceinline__ void load(const unsigned short* p, float (&v)[4]) { VT<unsigned short>::load4(p, v); }
    static __device__ __forceinline__ void store(unsigned short* p, const float (&v)[4]) { VT<unsigned short>::store4(p, v); }
};

// V in {1, 4, 8} consecutive floats of a contiguous fp32 array, 16 bytes at a time
template <int V>
__device__ __forceinline__ void load_f32(const float* p, float (&v)[V]) {
    if constexpr (V == 1) {
        v[0] = *p;
    } else {
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            const f32x4 t = reinterpret_cast<const f32x4*>(p)[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    }
}
template <int V>
__device__ __forceinline__ void store_f32(float* p, const float (&v)[V]) {
    if constexpr (V == 1) {
        *p = v[0];
    } else {
#pragma unroll
        for (int q = 0; q < V / 4; ++q) reinterpret_cast<f32x4*>(p)[q] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    }
}
}  // namespace
