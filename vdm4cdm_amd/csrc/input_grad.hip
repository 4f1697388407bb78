// input_grad.hip - K1t: input gradient of conv_in (the network's gradient w.r.t. z_t and s_conditioning).
//
// conv_in maps the two input channels {z, s_conditioning} to chs[0] channels with a 3x3x3 stride-1 pad-1 convolution, so its input
// gradient is a thin-output transposed convolution:
//     dz[n][q] = sum_{tap k} sum_c W[k][c][0] dh[n][q + 1 - k][c]          (ds: the same with W[k][c][1])
// with zeros or circular padding.  dh (NDHWC, C = chs[0] in {16, 32, 48, 64}, bf16 or fp32 storage) is read once from HBM; the outputs are
// fp32.  A workgroup owns a 4 x 4 x 16 tile of output voxels (one per thread) and stages the (6 x 6 x 18)-voxel halo of dh in LDS, 16
// channels at a time, as fp32 quads laid out [quad][voxel] (a wave reads 64 consecutive voxels' quads: no bank conflicts).  The weights
// are read with wave-uniform addresses.  Fixed summation order: bit-reproducible.  HBM floor: one read of dh + the fp32 outputs.
#include "common.h"

namespace vdm {

constexpr int IG_TZ = 4, IG_TY = 4, IG_TX = 16;                      // output tile (256 voxels, one per thread)
constexpr int IG_HZ = IG_TZ + 2, IG_HY = IG_TY + 2, IG_HX = IG_TX + 2;
constexpr int IG_HV = IG_HZ * IG_HY * IG_HX;                         // 648 halo voxels
constexpr int IG_CK = 16;                                            // channels per LDS pass (41.5 KB)

template <typename T> __device__ __forceinline__ float4 ld_quad(const T* p);
template <> __device__ __forceinline__ float4 ld_quad<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <> __device__ __forceinline__ float4 ld_quad<bf16_t>(const bf16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return make_float4(__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                       __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u));
}

__device__ __forceinline__ int wrap_idx(int g, int n) {
    const int r = g % n;
    return r < 0 ? r + n : r;
}

// K1t for conv_in's CIN = 1 + K <= 4 input channels (K conditioning fields, ABI v18).  Summation order per output: taps, then channel
// quads, then the four channels of a quad.  NACC = 1 computes dz alone, NACC = CIN also the K planes of ds [n][K][d][h][w] (K = 1: the
// [n][d][h][w] of vdm_conv_in_dgrad).  Both entries launch this kernel.
template <typename T, int CIN, int NACC>
__global__ void __launch_bounds__(256) conv_in_dgrad_fields_kernel(const T* __restrict__ dh, int C, int D, int H, int W, int circ,
                                                                   const float* __restrict__ wt, float* __restrict__ dz, float* __restrict__ ds,
                                                                   int tiles_x, int tiles_y, int tiles_z) {
    __shared__ float4 img[IG_CK / 4][IG_HV];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y;
    b /= tiles_y;
    const int tz = b % tiles_z;
    const int n = b / tiles_z;
    const int x0 = tx * IG_TX, y0 = ty * IG_TY, z0 = tz * IG_TZ;
    const int lx = tid % IG_TX, ly = (tid / IG_TX) % IG_TY, lz = tid / (IG_TX * IG_TY);
    const size_t vol = (size_t)D * H * W, nbase = (size_t)n * vol;
    float acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = 0.f;
    for (int c0 = 0; c0 < C; c0 += IG_CK) {
        __syncthreads();
        for (int e = tid; e < IG_HV * (IG_CK / 4); e += 256) {
            const int q = e % (IG_CK / 4), hv = e / (IG_CK / 4);
            const int hx = hv % IG_HX, hy = (hv / IG_HX) % IG_HY, hz = hv / (IG_HX * IG_HY);
            int gx = x0 - 1 + hx, gy = y0 - 1 + hy, gz = z0 - 1 + hz;
            bool ok;
            if (circ) {
                gx = wrap_idx(gx, W); gy = wrap_idx(gy, H); gz = wrap_idx(gz, D);
                ok = true;
            } else {
                ok = gx >= 0 && gx < W && gy >= 0 && gy < H && gz >= 0 && gz < D;
            }
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) v = ld_quad<T>(dh + (nbase + ((size_t)gz * H + gy) * W + gx) * C + c0 + 4 * q);
            img[q][hv] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kz = 0; kz < 3; ++kz)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int hv = ((lz + 2 - kz) * IG_HY + (ly + 2 - ky)) * IG_HX + (lx + 2 - kx);
                    const float* w = wt + ((size_t)((kz * 3 + ky) * 3 + kx) * C + c0) * CIN;
#pragma unroll
                    for (int q = 0; q < IG_CK / 4; ++q) {
                        const float4 v = img[q][hv];
                        const float* wq = w + 4 * q * CIN;
#pragma unroll
                        for (int a = 0; a < NACC; ++a) {
                            acc[a] = fmaf(v.x, wq[a], acc[a]); acc[a] = fmaf(v.y, wq[CIN + a], acc[a]);
                            acc[a] = fmaf(v.z, wq[2 * CIN + a], acc[a]); acc[a] = fmaf(v.w, wq[3 * CIN + a], acc[a]);
                        }
                    }
                }
    }
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    if (x < W && y < H && z < D) {
        const size_t o = ((size_t)z * H + y) * W + x;
        dz[nbase + o] = acc[0];
#pragma unroll
        for (int a = 1; a < NACC; ++a) ds[((size_t)n * (NACC - 1) + (a - 1)) * vol + o] = acc[a];
    }
}

}  // namespace vdm

using namespace vdm;

template <typename T, int CIN>
static void launch_dgrad_fields(bool with_ds, dim3 grid, hipStream_t s, const void* dh, int c, int d, int h, int w, int circ, const float* weight,
                                float* dz, float* ds, int tx, int ty, int tz) {
    if (with_ds)
        hipLaunchKernelGGL((conv_in_dgrad_fields_kernel<T, CIN, CIN>), grid, dim3(256), 0, s, (const T*)dh, c, d, h, w, circ, weight, dz, ds, tx, ty, tz);
    else
        hipLaunchKernelGGL((conv_in_dgrad_fields_kernel<T, CIN, 1>), grid, dim3(256), 0, s, (const T*)dh, c, d, h, w, circ, weight, dz, ds, tx, ty, tz);
}

template <typename T>
static void launch_dgrad_fields_cin(int cin, bool with_ds, dim3 grid, hipStream_t s, const void* dh, int c, int d, int h, int w, int circ,
                                    const float* weight, float* dz, float* ds, int tx, int ty, int tz) {
    if (cin == 1) launch_dgrad_fields<T, 1>(false, grid, s, dh, c, d, h, w, circ, weight, dz, ds, tx, ty, tz);
    else if (cin == 2) launch_dgrad_fields<T, 2>(with_ds, grid, s, dh, c, d, h, w, circ, weight, dz, ds, tx, ty, tz);
    else if (cin == 3) launch_dgrad_fields<T, 3>(with_ds, grid, s, dh, c, d, h, w, circ, weight, dz, ds, tx, ty, tz);
    else launch_dgrad_fields<T, 4>(with_ds, grid, s, dh, c, d, h, w, circ, weight, dz, ds, tx, ty, tz);
}

extern "C" int vdm_conv_in_dgrad(const void* dh, int n, int d, int h, int w, int c, int dtype, int pad_mode, const float* weight, int cin,
                                 float* dz, float* ds, void* stream) {
    VDM_REQUIRE(dh && weight && dz, "conv_in_dgrad: NULL pointer (dh, weight and dz are required)");
    VDM_REQUIRE(n > 0 && d > 0 && h > 0 && w > 0, "conv_in_dgrad: bad grid n=%d d=%d h=%d w=%d", n, d, h, w);
    VDM_REQUIRE(c == 16 || c == 32 || c == 48 || c == 64, "conv_in_dgrad: channels %d out of range (16, 32, 48 or 64)", c);
    VDM_REQUIRE(cin == 1 || cin == 2, "conv_in_dgrad: input channels %d out of range (1 or 2)", cin);
    VDM_REQUIRE(!ds || cin == 2, "conv_in_dgrad: ds needs cin == 2");
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "conv_in_dgrad: bad dtype %d", dtype);
    VDM_REQUIRE(pad_mode == VDM_PAD_ZEROS || pad_mode == VDM_PAD_CIRCULAR, "conv_in_dgrad: bad pad_mode %d", pad_mode);
    VDM_REQUIRE(((uintptr_t)dh & 15) == 0 && ((uintptr_t)weight & 3) == 0 && ((uintptr_t)dz & 3) == 0 && ((uintptr_t)ds & 3) == 0,
                "conv_in_dgrad: dh must be 16-byte aligned, weight / dz / ds 4-byte aligned");
    const int tx = (w + IG_TX - 1) / IG_TX, ty = (h + IG_TY - 1) / IG_TY, tz = (d + IG_TZ - 1) / IG_TZ;
    const long long blocks = (long long)tx * ty * tz * n;
    VDM_REQUIRE(blocks <= 0x7fffffffLL, "conv_in_dgrad: grid too large");
    hipStream_t s = (hipStream_t)stream;
    const int circ = pad_mode == VDM_PAD_CIRCULAR;
    const dim3 grid((unsigned)blocks);
    if (dtype == VDM_F32) launch_dgrad_fields_cin<float>(cin, ds != nullptr, grid, s, dh, c, d, h, w, circ, weight, dz, ds, tx, ty, tz);
    else launch_dgrad_fields_cin<bf16_t>(cin, ds != nullptr, grid, s, dh, c, d, h, w, circ, weight, dz, ds, tx, ty, tz);
    VDM_LAUNCH_CHECK("conv_in_dgrad_fields_kernel");
    return VDM_OK;
}

extern "C" int vdm_conv_in_dgrad_fields(const void* dh, int n, int d, int h, int w, int c, int dtype, int pad_mode, const float* weight, int cin,
                                        float* dz, float* ds, int n_ds, void* stream) {
    VDM_REQUIRE(dh && weight && dz, "conv_in_dgrad_fields: NULL pointer (dh, weight and dz are required)");
    VDM_REQUIRE(n > 0 && d > 0 && h > 0 && w > 0, "conv_in_dgrad_fields: bad grid n=%d d=%d h=%d w=%d", n, d, h, w);
    VDM_REQUIRE(c == 16 || c == 32 || c == 48 || c == 64, "conv_in_dgrad_fields: channels %d out of range (16, 32, 48 or 64)", c);
    VDM_REQUIRE(cin >= 1 && cin <= 4, "conv_in_dgrad_fields: input channels %d out of range (1 to 4)", cin);
    VDM_REQUIRE(n_ds == 0 || n_ds == cin - 1, "conv_in_dgrad_fields: n_ds=%d must be 0 or cin - 1 = %d", n_ds, cin - 1);
    VDM_REQUIRE(n_ds == 0 || ds, "conv_in_dgrad_fields: ds is NULL with n_ds=%d", n_ds);
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "conv_in_dgrad_fields: bad dtype %d", dtype);
    VDM_REQUIRE(pad_mode == VDM_PAD_ZEROS || pad_mode == VDM_PAD_CIRCULAR, "conv_in_dgrad_fields: bad pad_mode %d", pad_mode);
    VDM_REQUIRE(((uintptr_t)dh & 15) == 0 && ((uintptr_t)weight & 3) == 0 && ((uintptr_t)dz & 3) == 0 && ((uintptr_t)ds & 3) == 0,
                "conv_in_dgrad_fields: dh must be 16-byte aligned, weight / dz / ds 4-byte aligned");
    const int tx = (w + IG_TX - 1) / IG_TX, ty = (h + IG_TY - 1) / IG_TY, tz = (d + IG_TZ - 1) / IG_TZ;
    const long long blocks = (long long)tx * ty * tz * n;
    VDM_REQUIRE(blocks <= 0x7fffffffLL, "conv_in_dgrad_fields: grid too large");
    hipStream_t s = (hipStream_t)stream;
    const int circ = pad_mode == VDM_PAD_CIRCULAR;
    const dim3 grid((unsigned)blocks);
    if (dtype == VDM_F32) launch_dgrad_fields_cin<float>(cin, n_ds > 0, grid, s, dh, c, d, h, w, circ, weight, dz, ds, tx, ty, tz);
    else launch_dgrad_fields_cin<bf16_t>(cin, n_ds > 0, grid, s, dh, c, d, h, w, circ, weight, dz, ds, tx, ty, tz);
    VDM_LAUNCH_CHECK("conv_in_dgrad_fields_kernel");
    return VDM_OK;
}
