// field_stats.hip - the last data-preparation step on the device: the moments of log10(field + alpha) over a resident slab of a CAMELS
// stack, from which the normalisation constants (mean, population std) of a field are merged on the host.
//
// Replaces the arithmetic of the reference's notebook, scripts/calc_normalization.ipynb:
//   data = np.load(path).astype(np.float64); data = np.log10(data + alpha); m = data.mean(); s = data.std()
// which holds the whole stack twice in host memory.  Here one streaming pass per uploaded slab returns
//   {n_valid, S1 = sum(v - pivot), S2 = sum((v - pivot)^2), min x, max x, n_bad},   v = log10((double)x + alpha) in float64,
// over the valid elements (x finite and x + alpha > 0; the others are counted in n_bad and excluded).  With the pivot near the mean,
// S2/N - (S1/N)^2 has no cancellation to speak of, and records of different slabs computed with one pivot simply add.
//
// Bound: the fp64 VALU, not HBM: log10 in float64 is some tens of fp64 instructions per element against 4 bytes
// read.  So the loop is kept free of anything but the loads, the logarithm and the accumulation: validity is two compares and selects
// (no branch), the counts are 32-bit integer adds, min / max stay fp32, and the launch fills every SIMD with 8 waves so that the
// latency of the dependent fp64 chains is hidden by other waves.
//
// Determinism: thread t of the grid owns the groups of four elements t, t + T, t + 2T, ... (T threads, the grid a function of n
// alone) and adds them in that order; the wave is reduced with shuffles in a fixed pattern, the waves through LDS in index order, each
// workgroup writes one record, and a second launch of one workgroup adds the records in a fixed order.  No atomics.  A pointer that
// is not 16-byte aligned changes the load instructions, never the element-to-thread map: the result has the same bits.
#include "common.h"

#include <cmath>

namespace vdm {

constexpr int LM_THREADS = 256, LM_WAVES = LM_THREADS / 64;
constexpr int LM_GROUPS_PER_THREAD = 4;                     // a workgroup is added to the grid per LM_THREADS * 4 * this many elements
constexpr int LM_MAX_BLOCKS = VDM_LOG_MOMENTS_WS / VDM_LOG_MOMENTS_OUT;      // 2048: 8 workgroups of 4 waves on each of 256 CUs

struct Moments {
    double s1, s2;
    float lo, hi;
    uint32_t n_valid, n_bad;                                // per thread: at most n / (2048 * 256) + 4 elements (n <= 2^40: below 2^22)
};

__device__ __forceinline__ void lm_add(Moments& m, float x, double alpha, double pivot) {
    const double t = (double)x + alpha;
    const bool ok = fabsf(x) < INFINITY && t > 0.0;          // (NaN fails both compares)
    const double d = ok ? log10(t) - pivot : 0.0;
    m.s1 += d;
    m.s2 = fma(d, d, m.s2);
    m.lo = fminf(m.lo, ok ? x : INFINITY);
    m.hi = fmaxf(m.hi, ok ? x : -INFINITY);
    m.n_valid += ok ? 1u : 0u;
    m.n_bad += ok ? 0u : 1u;
}

// One record {n_valid, S1, S2, min, max, n_bad} of the whole workgroup, written by thread 0: shuffles inside the wave, then the waves
// in index order.
__device__ __forceinline__ void lm_block_reduce(double v[VDM_LOG_MOMENTS_OUT], double* __restrict__ record) {
    __shared__ double part[LM_WAVES][VDM_LOG_MOMENTS_OUT];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double a0 = __shfl_xor(v[0], o, 64), a1 = __shfl_xor(v[1], o, 64), a2 = __shfl_xor(v[2], o, 64);
        const double a3 = __shfl_xor(v[3], o, 64), a4 = __shfl_xor(v[4], o, 64), a5 = __shfl_xor(v[5], o, 64);
        v[0] += a0, v[1] += a1, v[2] += a2, v[3] = fmin(v[3], a3), v[4] = fmax(v[4], a4), v[5] += a5;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < VDM_LOG_MOMENTS_OUT; ++j) part[w][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[VDM_LOG_MOMENTS_OUT];
#pragma unroll
        for (int j = 0; j < VDM_LOG_MOMENTS_OUT; ++j) r[j] = part[0][j];
        for (int k = 1; k < LM_WAVES; ++k)
            r[0] += part[k][0], r[1] += part[k][1], r[2] += part[k][2], r[3] = fmin(r[3], part[k][3]), r[4] = fmax(r[4], part[k][4]),
                r[5] += part[k][5];
#pragma unroll
        for (int j = 0; j < VDM_LOG_MOMENTS_OUT; ++j) record[j] = r[j];
    }
}

// grid: lm_blocks(n) workgroups; VEC: x is 16-byte aligned (the full groups are read with one 16-byte load each)
template <bool VEC>
__global__ void __launch_bounds__(LM_THREADS) log_moments_kernel(const float* __restrict__ x, int64_t n, double alpha, double pivot,
                                                                 double* __restrict__ records) {
    Moments m = {0.0, 0.0, INFINITY, -INFINITY, 0u, 0u};
    const int64_t tid = (int64_t)blockIdx.x * LM_THREADS + threadIdx.x, threads = (int64_t)gridDim.x * LM_THREADS;
    const int64_t full = n >> 2;                            // groups of four whole elements
    for (int64_t g = tid; g < full; g += threads) {
        float4 q;
        if (VEC) {
            q = *reinterpret_cast<const float4*>(x + 4 * g);
        } else {
            const float* p = x + 4 * g;
            q = make_float4(p[0], p[1], p[2], p[3]);
        }
        lm_add(m, q.x, alpha, pivot);
        lm_add(m, q.y, alpha, pivot);
        lm_add(m, q.z, alpha, pivot);
        lm_add(m, q.w, alpha, pivot);
    }
    if ((n & 3) && full % threads == tid)                    // the ragged last group belongs to the thread whose turn it is
        for (int64_t i = 4 * full; i < n; ++i) lm_add(m, x[i], alpha, pivot);
    double v[VDM_LOG_MOMENTS_OUT] = {(double)m.n_valid, m.s1, m.s2, (double)m.lo, (double)m.hi, (double)m.n_bad};
    lm_block_reduce(v, records + (size_t)blockIdx.x * VDM_LOG_MOMENTS_OUT);
}

// one workgroup: thread t adds the records t * per, ..., t * per + per - 1 in index order, then the workgroup reduction of above
__global__ void __launch_bounds__(LM_THREADS) log_moments_final_kernel(const double* __restrict__ records, int n_records,
                                                                       double* __restrict__ out) {
    const int per = (n_records + LM_THREADS - 1) / LM_THREADS;
    double v[VDM_LOG_MOMENTS_OUT] = {0.0, 0.0, 0.0, (double)INFINITY, -(double)INFINITY, 0.0};
    for (int r = threadIdx.x * per; r < min((int)(threadIdx.x + 1) * per, n_records); ++r) {
        const double* p = records + (size_t)r * VDM_LOG_MOMENTS_OUT;
        v[0] += p[0], v[1] += p[1], v[2] += p[2], v[3] = fmin(v[3], p[3]), v[4] = fmax(v[4], p[4]), v[5] += p[5];
    }
    lm_block_reduce(v, out);
}

static int lm_blocks(int64_t n) {
    const int64_t per_block = (int64_t)LM_THREADS * 4 * LM_GROUPS_PER_THREAD;
    const int64_t b = (n + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > LM_MAX_BLOCKS ? LM_MAX_BLOCKS : b);
}

}  // namespace vdm

using namespace vdm;

extern "C" int vdm_log_moments(const float* x, int64_t n, double alpha, double pivot, double* out, double* workspace, void* stream) {
    static_assert(LM_MAX_BLOCKS * VDM_LOG_MOMENTS_OUT == VDM_LOG_MOMENTS_WS && LM_MAX_BLOCKS >= 1, "workspace = whole records");
    VDM_REQUIRE(x, "log_moments: x is NULL");
    VDM_REQUIRE(out, "log_moments: out is NULL");
    VDM_REQUIRE(workspace, "log_moments: workspace is NULL");
    VDM_REQUIRE(n >= 0, "log_moments: n = %lld is negative", (long long)n);
    VDM_REQUIRE(n <= ((int64_t)1 << 40), "log_moments: n = %lld exceeds 2^40 elements per call", (long long)n);
    VDM_REQUIRE(std::isfinite(alpha), "log_moments: alpha = %g is not finite", alpha);
    VDM_REQUIRE(std::isfinite(pivot), "log_moments: pivot = %g is not finite", pivot);
    // (n == 0 runs the same two launches: no thread finds an element, and the empty record {0, 0, 0, +inf, -inf, 0} comes out)
    const int blocks = lm_blocks(n);
    if (reinterpret_cast<uintptr_t>(x) % 16 == 0)
        hipLaunchKernelGGL(log_moments_kernel<true>, dim3(blocks), dim3(LM_THREADS), 0, (hipStream_t)stream, x, n, alpha, pivot, workspace);
    else
        hipLaunchKernelGGL(log_moments_kernel<false>, dim3(blocks), dim3(LM_THREADS), 0, (hipStream_t)stream, x, n, alpha, pivot, workspace);
    VDM_LAUNCH_CHECK("log_moments_kernel");
    hipLaunchKernelGGL(log_moments_final_kernel, dim3(1), dim3(LM_THREADS), 0, (hipStream_t)stream, workspace, blocks, out);
    VDM_LAUNCH_CHECK("log_moments_final_kernel");
    return VDM_OK;
}
