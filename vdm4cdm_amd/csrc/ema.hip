// ema.hip - exponential moving average of the weights: the one streaming pass a training step adds (vdm_ema_update) and the in-place
// exchange of two vectors that evaluation under the averaged weights uses (vdm_swap).  Both are HBM-bound grid-stride kernels over fp32
// vectors: float4 accesses when both pointers are 16-byte aligned (ragged tail scalar), fully scalar otherwise (the schedule scalars,
// n = 1, sit wherever the allocator put them).
#include "common.h"

namespace vdm {

static inline unsigned ema_grid(int64_t work_items) {
    int64_t g = (work_items + 255) / 256;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;          // ~8 blocks/CU; grid-stride the rest
    return (unsigned)g;
}

// The arithmetic is pinned so that a float32 reference that rounds every operation on its own reproduces it bit for bit:
//   q  = rn((float)(1 + k) / (float)(10 + k))     (integer sums first, each converted once)
//   d  = warmup ? min(decay, q) : decay
//   w  = rn(1 - d)
//   e' = rn(e + rn(w * rn(p - e)))
// The build contracts a * b + c into one FMA (-ffp-contract=fast) and the _rn intrinsics of this toolchain are plain inline operators,
// so the product additionally goes through uncontracted_mul: no FMA can form.  The kernel is memory bound; the extra rounding is free.
__device__ __forceinline__ float ema_weight(float decay, int warmup, const int32_t* num_updates) {
    float d = decay;
    if (warmup) {
        const int64_t k = num_updates ? (int64_t)*num_updates : 0;
        const float q = __fdiv_rn((float)(1 + k), (float)(10 + k));
        d = fminf(decay, q);
    }
    return __fsub_rn(1.0f, d);
}

__device__ __forceinline__ float ema_one(float e, float p, float w) { return __fadd_rn(e, uncontracted_mul(w, __fsub_rn(p, e))); }

// n4: float4 groups handled vectorised (0 when a pointer is not 16-byte aligned); [4 * n4, n) is the scalar part.
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n4, int64_t n,
                                                         float decay, int warmup, const int32_t* __restrict__ num_updates) {
    const float w = ema_weight(decay, warmup, num_updates);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    float4* e4 = reinterpret_cast<float4*>(ema);
    const float4* p4 = reinterpret_cast<const float4*>(p);
    for (int64_t i = tid; i < n4; i += stride) {
        float4 e = e4[i];
        const float4 v = p4[i];
        e.x = ema_one(e.x, v.x, w);
        e.y = ema_one(e.y, v.y, w);
        e.z = ema_one(e.z, v.z, w);
        e.w = ema_one(e.w, v.w, w);
        e4[i] = e;
    }
    for (int64_t i = 4 * n4 + tid; i < n; i += stride) ema[i] = ema_one(ema[i], p[i], w);
}

__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n4, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    float4* a4 = reinterpret_cast<float4*>(a);
    float4* b4 = reinterpret_cast<float4*>(b);
    for (int64_t i = tid; i < n4; i += stride) {
        const float4 x = a4[i], y = b4[i];
        a4[i] = y;
        b4[i] = x;
    }
    for (int64_t i = 4 * n4 + tid; i < n; i += stride) {
        const float x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

}  // namespace vdm

using namespace vdm;

extern "C" int vdm_ema_update(float* ema, const float* p, int64_t n, float decay, int warmup, const int32_t* num_updates, void* stream) {
    VDM_REQUIRE(ema && p, "ema_update: NULL pointer (ema and p are required)");
    VDM_REQUIRE(n >= 0, "ema_update: n = %lld (must not be negative)", (long long)n);
    VDM_REQUIRE(decay >= 0.f && decay < 1.f, "ema_update: decay = %g is not a finite number in [0, 1)", (double)decay);      // (refuses NaN too)
    VDM_REQUIRE((const float*)ema != p, "ema_update: ema and p are the same vector");
    VDM_REQUIRE((((uintptr_t)ema | (uintptr_t)p | (uintptr_t)num_updates) & 3) == 0, "ema_update: ema, p and num_updates must be 4-byte aligned");
    if (n == 0) return VDM_OK;
    const int64_t n4 = (((uintptr_t)ema | (uintptr_t)p) & 15) == 0 ? n >> 2 : 0;
    hipLaunchKernelGGL(ema_update_kernel, dim3(ema_grid(n4 ? n4 : n)), dim3(256), 0, (hipStream_t)stream, ema, p, n4, n, decay, warmup != 0,
                       num_updates);
    VDM_LAUNCH_CHECK("ema_update_kernel");
    return VDM_OK;
}

extern "C" int vdm_swap(float* a, float* b, int64_t n, void* stream) {
    VDM_REQUIRE(a && b, "swap: NULL pointer (a and b are required)");
    VDM_REQUIRE(n >= 0, "swap: n = %lld (must not be negative)", (long long)n);
    VDM_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 3) == 0, "swap: a and b must be 4-byte aligned");
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
    VDM_REQUIRE(ua != ub && (ua < ub ? ub - ua >= bytes : ua - ub >= bytes), "swap: the ranges [a, a + n) and [b, b + n) overlap");
    if (n == 0) return VDM_OK;
    const int64_t n4 = ((ua | ub) & 15) == 0 ? n >> 2 : 0;
    hipLaunchKernelGGL(swap_kernel, dim3(ema_grid(n4 ? n4 : n)), dim3(256), 0, (hipStream_t)stream, a, b, n4, n);
    VDM_LAUNCH_CHECK("swap_kernel");
    return VDM_OK;
}
