// Small streaming kernels (HBM-bound, 16 B per lane where alignment allows).
#include "common.h"
#include "vec16.h"

namespace {

template <typename T, bool VEC>
__global__ void __launch_bounds__(256) mix_rows_kernel(const T* x, const int64_t* perm, float lam, int64_t n, T* out) {
    const int b = blockIdx.y;
    const T* xa = x + (int64_t)b * n;
    const T* xb = x + perm[b] * n;
    T* o = out + (int64_t)b * n;
    const float mu = 1.0f - lam;
    constexpr int N = VT<T>::V;
    if (VEC) {
        for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * N; i < n; i += (int64_t)gridDim.x * 256 * N) {
            float a[N], c[N];
            VT<T>::load(xa + i, a); VT<T>::load(xb + i, c);
#pragma unroll
            for (int k = 0; k < N; ++k) a[k] = lam * a[k] + mu * c[k];
            VT<T>::store(o + i, a);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
            VT<T>::store1(o + i, lam * VT<T>::load1(xa + i) + mu * VT<T>::load1(xb + i));
    }
}

}  // namespace

extern "C" int iif_mix_rows(const void* x, int dtype, const int64_t* perm, float lam, int B, int64_t n, void* out,
                            void* stream) {
    if (B < 0 || n < 0) return IIF_EINVAL;
    if (B == 0 || n == 0) return IIF_OK;
    if (!x || !perm || !out || B > 65535) return IIF_EINVAL;
    hipStream_t st = as_stream(stream);
    const bool al = (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    if (dtype == IIF_F32) {
        const bool vec = al && (n % 4 == 0);
        const int gx = (int)(cdiv64(n, vec ? 1024 : 256) < 64 ? cdiv64(n, vec ? 1024 : 256) : 64);
        if (vec) hipLaunchKernelGGL((mix_rows_kernel<float, true>), dim3(gx, B), dim3(256), 0, st, (const float*)x, perm, lam, n, (float*)out);
        else hipLaunchKernelGGL((mix_rows_kernel<float, false>), dim3(gx, B), dim3(256), 0, st, (const float*)x, perm, lam, n, (float*)out);
    } else if (dtype == IIF_BF16) {
        const bool vec = al && (n % 8 == 0);
        const int gx = (int)(cdiv64(n, vec ? 2048 : 256) < 64 ? cdiv64(n, vec ? 2048 : 256) : 64);
        if (vec) hipLaunchKernelGGL((mix_rows_kernel<unsigned short, true>), dim3(gx, B), dim3(256), 0, st, (const unsigned short*)x, perm, lam, n, (unsigned short*)out);
        else hipLaunchKernelGGL((mix_rows_kernel<unsigned short, false>), dim3(gx, B), dim3(256), 0, st, (const unsigned short*)x, perm, lam, n, (unsigned short*)out);
    } else {
        return IIF_EINVAL;
    }
    IIF_LAUNCH_CHECK();
    return IIF_OK;
}
