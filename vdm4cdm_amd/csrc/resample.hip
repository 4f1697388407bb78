// resample.hip - the data-preparation step on the device: the 256^3 CAMELS cube stacks down-gridded to the training sizes (128 ... 224)
// by trilinear interpolation, one launch per resident slab of cubes.
//
// Replaces the data-preparation notebook of the reference, scripts/make_down_grids.ipynb cell 3:
//   torch.nn.functional.interpolate(stack[:, None], size=T, mode="trilinear", align_corners=False)
// per axis and output index d: source coordinate max((d + 1/2) S/T - 1/2, 0), i0 = floor, i1 = min(i0 + 1, S - 1), lambda = frac; edges
// are clamped, not periodic.  Index and weight come from the exact rational ((2d + 1) S - T) / (2T) in integer arithmetic (quotient =
// i0, remainder / 2T rounded once to fp32 = lambda), so the result does not depend on how a float evaluation of the coordinate rounds.
//
// Bound: HBM, (S^3 + T^3) * 4 B per cube.  An output row (z, y) blends four input rows (z0|z1, y0|y1).  One wave owns one output row:
// it reads its four input rows along x (16 bytes per lane, whole rows), blends them in z and then y into ONE row of S floats in LDS,
// and gathers that row in x for a 16-byte store of four outputs per lane.  The four waves of a workgroup own four neighbouring y of
// one z: the input rows they share are served by the CU's vector cache, the rows shared with the z-neighbours by L2.
// Blend order is fixed (z, then y, then x; each fma(l, b, (1 - l) a)); no atomics: the same input gives the same bits on every call.
#include "common.h"

namespace vdm {

constexpr int RS_ROWS = 4, RS_MAX = 1024;                  // output rows (waves) per workgroup; largest edge

struct Tap { int i0, i1; float l; };

// (i0, i1, lambda) of output index d along one axis: ((2d + 1) S - T) / (2T), exact (the numerator is below 2^22 for S <= 1024)
__device__ __forceinline__ Tap tap_of(int d, int S, int T, const FastDiv& by2T) {
    const int num = max((2 * d + 1) * S - T, 0);
    const int q = (int)fdiv((uint32_t)num, by2T);
    Tap t;
    t.i0 = q;
    t.i1 = min(q + 1, S - 1);
    t.l = (float)(num - q * 2 * T) / (float)(2 * T);      // both operands exact in fp32: one correctly rounded division
    return t;
}

// lambda == 0 returns `a` itself (T == S is a bit-exact copy, also of -0 and next to a non-finite neighbour)
__device__ __forceinline__ float blend(float a, float b, float l) { return l == 0.f ? a : fmaf(l, b, (1.f - l) * a); }

__device__ __forceinline__ float blend_zy(float a00, float a10, float a01, float a11, float lz, float ly) {
    return blend(blend(a00, a10, lz), blend(a01, a11, lz), ly);
}

// grid (ceil(T / RS_ROWS), T, cubes); VEC: S % 4 == 0, T % 4 == 0 and both pointers 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(64 * RS_ROWS) downgrid_kernel(const float* __restrict__ src, float* __restrict__ dst, int S, int T,
                                                                const FastDiv by2T) {
    __shared__ __attribute__((aligned(16))) float rows[RS_ROWS][RS_MAX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int y = blockIdx.x * RS_ROWS + w, z = blockIdx.y;
    const size_t cube = blockIdx.z;
    const bool live = y < T;                                // (no early return: every wave reaches the barrier)
    float* row = rows[w];
    if (live) {
        const Tap tz = tap_of(z, S, T, by2T), ty = tap_of(y, S, T, by2T);
        const float* p = src + cube * S * S * S;
        const float* r00 = p + ((size_t)tz.i0 * S + ty.i0) * S;
        const float* r01 = p + ((size_t)tz.i0 * S + ty.i1) * S;
        const float* r10 = p + ((size_t)tz.i1 * S + ty.i0) * S;
        const float* r11 = p + ((size_t)tz.i1 * S + ty.i1) * S;
        if (VEC) {
            for (int x = lane * 4; x < S; x += 256) {
                const float4 a00 = *reinterpret_cast<const float4*>(r00 + x), a01 = *reinterpret_cast<const float4*>(r01 + x);
                const float4 a10 = *reinterpret_cast<const float4*>(r10 + x), a11 = *reinterpret_cast<const float4*>(r11 + x);
                float4 o;
                o.x = blend_zy(a00.x, a10.x, a01.x, a11.x, tz.l, ty.l);
                o.y = blend_zy(a00.y, a10.y, a01.y, a11.y, tz.l, ty.l);
                o.z = blend_zy(a00.z, a10.z, a01.z, a11.z, tz.l, ty.l);
                o.w = blend_zy(a00.w, a10.w, a01.w, a11.w, tz.l, ty.l);
                *reinterpret_cast<float4*>(row + x) = o;
            }
        } else {
            for (int x = lane; x < S; x += 64) row[x] = blend_zy(r00[x], r10[x], r01[x], r11[x], tz.l, ty.l);
        }
    }
    __syncthreads();
    if (live) {
        float* o = dst + ((cube * T + z) * T + y) * T;
        if (VEC) {
            for (int x = lane * 4; x < T; x += 256) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const Tap tx = tap_of(x + j, S, T, by2T);
                    v[j] = blend(row[tx.i0], row[tx.i1], tx.l);
                }
                *reinterpret_cast<float4*>(o + x) = make_float4(v[0], v[1], v[2], v[3]);
            }
        } else {
            for (int x = lane; x < T; x += 64) {
                const Tap tx = tap_of(x, S, T, by2T);
                o[x] = blend(row[tx.i0], row[tx.i1], tx.l);
            }
        }
    }
}

}  // namespace vdm

using namespace vdm;

extern "C" int vdm_downgrid_trilinear(const float* src, float* dst, int64_t n, int S, int T, void* stream) {
    VDM_REQUIRE(src, "downgrid_trilinear: src is NULL");
    VDM_REQUIRE(dst, "downgrid_trilinear: dst is NULL");
    VDM_REQUIRE(n >= 0, "downgrid_trilinear: n = %lld is negative", (long long)n);
    VDM_REQUIRE(S >= 1 && S <= RS_MAX, "downgrid_trilinear: S = %d is outside 1..%d", S, RS_MAX);
    VDM_REQUIRE(T >= 1 && T <= RS_MAX, "downgrid_trilinear: T = %d is outside 1..%d", T, RS_MAX);
    VDM_REQUIRE(T <= S, "downgrid_trilinear: T = %d exceeds S = %d (up-sampling is not supported)", T, S);
    if (n == 0) return VDM_OK;
    const FastDiv by2T = make_fastdiv((uint32_t)(2 * T));
    const bool vec = S % 4 == 0 && T % 4 == 0 && (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16 == 0;
    const size_t s3 = (size_t)S * S * S, t3 = (size_t)T * T * T;
    const int64_t chunk = 32768;                            // cubes per launch (grid.z)
    for (int64_t n0 = 0; n0 < n; n0 += chunk) {
        const int nc = (int)(n - n0 < chunk ? n - n0 : chunk);
        const dim3 grid((T + RS_ROWS - 1) / RS_ROWS, T, nc);
        if (vec)
            hipLaunchKernelGGL(downgrid_kernel<true>, grid, dim3(64 * RS_ROWS), 0, (hipStream_t)stream, src + n0 * s3, dst + n0 * t3, S, T, by2T);
        else
            hipLaunchKernelGGL(downgrid_kernel<false>, grid, dim3(64 * RS_ROWS), 0, (hipStream_t)stream, src + n0 * s3, dst + n0 * t3, S, T, by2T);
        VDM_LAUNCH_CHECK("downgrid_kernel");
    }
    return VDM_OK;
}
