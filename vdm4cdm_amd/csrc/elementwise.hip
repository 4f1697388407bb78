// elementwise.hip - HBM-bound kernels of the VDM denoising path (K2, K7-K10 of DESIGN.md):
// GroupNorm statistics, fused GroupNorm-apply+SiLU(+dropout) forward/backward, VDM forward
// diffusion, ELBO reductions, ancestral update with Philox normals, gradient-norm reduction and
// the small layout helpers, and the scalar glue of the training step (time grid / ELBO assembly / clip scale).  All are
// 16-byte-vectorised NDHWC streams with wave64 shuffle reductions and fixed-order two-stage folds (no float atomics).
#include "common.h"

namespace vdm {

static inline unsigned grid_for(int64_t work_items, int per_block) {
    int64_t g = (work_items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;          // ~8 blocks/CU; grid-stride the rest
    return (unsigned)g;
}

// block-wide sum of NVAL values; result valid in thread 0.  256 threads = 4 waves.
template <int NVAL>
__device__ __forceinline__ void block_sum(float (&v)[NVAL], float* smem /* >= 4*NVAL floats */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NVAL; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NVAL; ++i) smem[wave * NVAL + i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NVAL; ++i) v[i] = smem[i] + smem[NVAL + i] + smem[2 * NVAL + i] + smem[3 * NVAL + i];
    }
}

// ---------------------------------------------------------------------------------------------
// GroupNorm statistics: stats[n][g] = {sum, sumsq}.  One source tensor [n][V][C] whose groups
// occupy [g0, g0 + C/gs) of the `G`-group concatenated tensor.
// Work split: thread t owns piece column pc = t % PPV (16 B of channels), rows t / PPV + k*RPB.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) gn_stats_kernel(const T* __restrict__ x, int C, int64_t V, int gs, int G, int g0,
                                                      float* __restrict__ partial, int blocks_per_n) {
    constexpr int EPL = DT<T>::EPL;
    const int n = blockIdx.x / blocks_per_n, bn = blockIdx.x % blocks_per_n;
    const int PPV = C / EPL;                       // pieces per voxel
    const int64_t npieces = V * PPV;
    const uint4* xp = reinterpret_cast<const uint4*>(x + (size_t)n * V * C);
    // a thread's channel piece is fixed when the stride is a multiple of PPV
    const int64_t stride = (int64_t)blocks_per_n * 256;
    // fast path: stride % PPV == 0 -> the piece column of a thread never changes
    float s[EPL], ss[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) s[j] = ss[j] = 0.f;
    const int64_t start = (int64_t)bn * 256 + threadIdx.x;
    for (int64_t i = start; i < npieces; i += stride) {
        Piece<T> p;
        p.load(xp[i]);
#pragma unroll
        for (int j = 0; j < EPL; ++j) { s[j] += p.f[j]; ss[j] += p.f[j] * p.f[j]; }
    }
    // Fixed-order block reduction (no float atomics: the forward pass must be bit-reproducible).
    __shared__ float sm[256 * EPL * 2];
    __shared__ float sh[2 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((64 % PPV) == 0) {
        // lanes with equal (lane % PPV) own the same piece column: xor-butterfly over the other lane bits,
        // then 4 waves x PPV columns x EPL channels go through LDS and 2G threads finish in channel order.
        for (int off = 32; off >= PPV; off >>= 1) {
#pragma unroll
            for (int j = 0; j < EPL; ++j) {
                s[j] += __shfl_xor(s[j], off, 64);
                ss[j] += __shfl_xor(ss[j], off, 64);
            }
        }
        if (lane < PPV) {
#pragma unroll
            for (int j = 0; j < EPL; ++j) {
                sm[((wave * PPV + lane) * EPL + j) * 2] = s[j];
                sm[((wave * PPV + lane) * EPL + j) * 2 + 1] = ss[j];
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * G) {
            const int g = (int)threadIdx.x >> 1, which = threadIdx.x & 1;
            float acc = 0.f;
            const int c_lo = (g - g0) * gs;
            if (g >= g0 && c_lo < C) {
                for (int c = c_lo; c < c_lo + gs; ++c)
                    for (int w = 0; w < 4; ++w) acc += sm[((w * PPV + c / EPL) * EPL + c % EPL) * 2 + which];
            }
            sh[threadIdx.x] = acc;
        }
    } else {
        // generic (e.g. 96 channels): every thread parks its sums; 2G threads walk the 256 entries in order.
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            sm[(threadIdx.x * EPL + j) * 2] = s[j];
            sm[(threadIdx.x * EPL + j) * 2 + 1] = ss[j];
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * G) {
            const int g = (int)threadIdx.x >> 1, which = threadIdx.x & 1;
            float acc = 0.f;
            const unsigned base = (unsigned)((int64_t)bn * 256 % PPV);
            for (int t = 0; t < 256; ++t) {
                const int c0 = (int)((base + t) % (unsigned)PPV) * EPL;
                if (g0 + c0 / gs > g || g0 + (c0 + EPL - 1) / gs < g) continue;
#pragma unroll
                for (int j = 0; j < EPL; ++j)
                    if (g0 + (c0 + j) / gs == g) acc += sm[(t * EPL + j) * 2 + which];
            }
            sh[threadIdx.x] = acc;
        }
    }
    __syncthreads();
    // per-block partials; gn_stats_finalize_kernel sums them in a fixed order (bit-reproducible forward)
    for (int i = threadIdx.x; i < 2 * G; i += 256) partial[((size_t)n * blocks_per_n + bn) * 2 * G + i] = sh[i];
}

// stats[n][g][0..1] = sum over blocks of partial, groups [g0, g0+gc) only.  One block per sample; thread (entry e, part k)
// sums every 256/NE-th block partial of its entry, then a fixed-order LDS fold over the parts (deterministic).
__global__ void __launch_bounds__(256) gn_stats_finalize_kernel(const float* __restrict__ partial, int G, int g0, int gc,
                                                               int blocks_per_n, float* __restrict__ stats) {
    const int n = blockIdx.x;
    const int NE = 2 * gc;                                   // entries to produce (<= 128)
    int parts = 256 / NE;
    if (parts < 1) parts = 1;
    const int e = threadIdx.x % NE, k = threadIdx.x / NE;
    __shared__ float sm[256];
    float s = 0.f;
    if (k < parts)
        for (int b = k; b < blocks_per_n; b += parts) s += partial[((size_t)n * blocks_per_n + b) * 2 * G + 2 * g0 + e];
    sm[threadIdx.x] = s;
    __syncthreads();
    if (k == 0 && (int)threadIdx.x < NE) {
        float tot = 0.f;
        for (int j = 0; j < parts; ++j) tot += sm[j * NE + e];
        stats[(size_t)n * 2 * G + 2 * g0 + e] = tot;
    }
}

// Sum of the per-tile channel partials a conv epilogue wrote (conv_common.h, gn_partials_reduce): p2[tile][C] (float2), channels
// [0, gs) of it -> sm[k][c] = sum over the tiles of component k of channel c, for c < gs (valid after the trailing barrier).
// Thread t owns channel t % gs and the tiles t / gs, t / gs + per, ...; U independent loads in flight per thread (the sweep is
// pure latency: the partials come from beyond the L2 of this XCD; in the step these launches take 3-45 us for the same work -
// their duration is the wait for free wave slots next to the other queues' kernels, which is why neither 16 or 32 loads in flight
// nor 1024-thread blocks - slower: a 16-wave block waits for a whole free CU - changed their average).  Power-of-two gs <= 64: the lanes of a wave that own the same
// channel are folded by an xor-butterfly, the waves through LDS in wave order; otherwise every thread parks its sums and gs
// threads walk them.  Both orders are fixed: bit-reproducible.
template <int NT>
__device__ __forceinline__ void tile_partials_fold(const float2* __restrict__ p2, int tiles, int C, int gs, float (*sm)[NT]) {
    const int per = NT / gs, S = per * gs;                  // tiles in flight per sweep, active threads
    const int t = threadIdx.x, c = t % gs, b0 = t / gs;
    float s0 = 0.f, s1 = 0.f;
    if (t < S) {
        constexpr int U = 16;
        for (int b = b0; b < tiles; b += per * U) {
            float2 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int bb = b + u * per;
                v[u] = bb < tiles ? p2[(size_t)bb * C + c] : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) { s0 += v[u].x; s1 += v[u].y; }
        }
    }
    if (gs <= 64 && (gs & (gs - 1)) == 0) {                 // (uniform)
        for (int off = 32; off >= gs; off >>= 1) {
            s0 += __shfl_xor(s0, off, 64);
            s1 += __shfl_xor(s1, off, 64);
        }
        const int lane = t & 63, wave = t >> 6;
        if (lane < gs) { sm[0][wave * gs + lane] = s0; sm[1][wave * gs + lane] = s1; }
        __syncthreads();
        float a0 = 0.f, a1 = 0.f;
        if (t < gs)
            for (int w = 0; w < NT / 64; ++w) { a0 += sm[0][w * gs + t]; a1 += sm[1][w * gs + t]; }
        __syncthreads();
        if (t < gs) { sm[0][t] = a0; sm[1][t] = a1; }
    } else {
        sm[0][t] = s0; sm[1][t] = s1;
        __syncthreads();
        if (t < gs) {                                       // (slot t < gs is only read by this thread)
            float a0 = 0.f, a1 = 0.f;
            for (int j = 0; j < per; ++j) { a0 += sm[0][t + j * gs]; a1 += sm[1][t + j * gs]; }
            sm[0][t] = a0; sm[1][t] = a1;
        }
    }
    __syncthreads();
}

// GroupNorm statistics from those partials: part[n][tile][C][2] -> stats[n][g0 + g][k] = sum over tiles and over the gs channels of
// group g.  One block per (sample, group).  chsum (optional): the per-channel sums chsum[n][c0 + c] = sum_v x[n][v][c] (the analytic
// column sums of the GroupNorm backward need them).
// Two sources (a skip concat whose halves were produced by two convs) in ONE launch: blocks [0, C / gs) of a sample take source 1,
// the following C2 / gs blocks source 2 (part2 == nullptr: one source).
template <int NT>
__global__ void __launch_bounds__(NT) gn_stats_from_partials_kernel(const float* __restrict__ part, int tiles, int C, int gs, int G,
                                                                    int g0, float* __restrict__ stats, float* __restrict__ chsum,
                                                                    int chsum_stride, int c0, const float* __restrict__ part2, int tiles2,
                                                                    int C2) {
    const int gc1 = C / gs, gcs = gc1 + (part2 ? C2 / gs : 0);
    const int n = blockIdx.x / gcs;
    int g = blockIdx.x % gcs;
    if (g >= gc1) {                                        // (uniform per block) second source: its groups follow the first one's
        g -= gc1; g0 += gc1; c0 += C;
        part = part2; tiles = tiles2; C = C2;
    }
    const float2* p2 = reinterpret_cast<const float2*>(part) + (size_t)n * tiles * C + (size_t)g * gs;
    __shared__ float sm[2][NT];
    tile_partials_fold<NT>(p2, tiles, C, gs, sm);
    const int t = threadIdx.x;
    if (chsum && t < gs) chsum[(size_t)n * chsum_stride + c0 + g * gs + t] = sm[0][t];
    if (t < 2) {
        float tot = 0.f;
        for (int j = 0; j < gs; ++j) tot += sm[t][j];
        stats[((size_t)n * G + g0 + g) * 2 + t] = tot;
    }
}

// per-(n, channel) affine of GN: y = x * A + B with A = rstd*gamma, B = beta - mean*rstd*gamma
__device__ __forceinline__ void gn_affine(const float* __restrict__ stats, int n, int G, int g, float cnt, float eps, float gamma,
                                          float beta, float& A, float& B, float& mean, float& rstd) {
    const float sum = stats[((size_t)n * G + g) * 2], sq = stats[((size_t)n * G + g) * 2 + 1];
    mean = sum / cnt;
    const float var = fmaxf(sq / cnt - mean * mean, 0.f);
    rstd = rsqrtf(var + eps);
    A = rstd * gamma;
    B = beta - mean * A;
}

// ---------------------------------------------------------------------------------------------
// y[n][v][c1+c2] = dropout(silu(gn(concat(x1,x2))))
// ---------------------------------------------------------------------------------------------
struct GnArgs {
    const void* x1; const void* x2;
    int c1, c2, n, G;
    int64_t V;
    const float* stats; const float* gamma; const float* beta;
    float eps, p;
    uint64_t seed;
    const int32_t* seed_step;   // optional DEVICE step counter mixed into the seed (a captured graph replays with fresh masks)
    void* y;                 // fwd out
    const void* dy; const void* add1; const void* add2; void* dx1; void* dx2;       // bwd
    long long colsum_stride;
    float* dgamma; float* dbeta; float* colsum; float* red;
    int blocks_per_n;
    unsigned char* mask;     // fwd (optional out): dropout keep bits, one byte per 16-byte piece of y
    const float* chan;       // bwd apply (fused path): per-sample channel sums [n][C][2] of (dyh, dyh*xhat)
    int linear;              // 1: no activation (plain GroupNorm, the attention block's norm); 0: SiLU
};

// effective RNG seed: the host seed, advanced by the device-side step counter when one is given - a hipGraph of the training step bakes
// the host seed into its kernel arguments, the counter (bumped once per replay) keeps the dropout masks / noise fields fresh
__device__ __forceinline__ uint64_t mix_seed(uint64_t seed, const int32_t* step) {
    return step ? seed + (uint64_t)(uint32_t)(*step) * 0x9E3779B97F4A7C15ull : seed;
}

// Dropout keep bits of one 16-byte piece (EPL elements) from ONE Philox4x32-10 block keyed by (seed, global piece index): fp32 storage
// (4 elements) takes 32 bits per element, bf16 storage (8 elements) 16 bits per element - keep iff the field exceeds p scaled to the
// field (|rate - p| < 8e-6 at 16 bits).  Round 4: was one Philox block per FOUR elements, i.e. two per bf16 piece - the generator was a
// third of the level-0 pass (153 vs 110 us with / without dropout).
template <int EPL>
__device__ __forceinline__ unsigned keep_bits_of_piece(uint64_t seed, uint64_t piece, float p) {
    uint32_t rnd[4];
    Philox::gen((uint32_t)piece, (uint32_t)(piece >> 32), 0x5eedu, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), rnd);
    unsigned bits = 0;
    if constexpr (EPL == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bits |= (u32_to_unit(rnd[j]) > p ? 1u : 0u) << j;
    } else {
        const uint32_t thr = (uint32_t)(p * 65536.0f + 0.5f);
#pragma unroll
        for (int j = 0; j < 8; ++j) bits |= ((((rnd[j >> 1] >> (16 * (j & 1))) & 0xffffu) >= thr) ? 1u : 0u) << j;
    }
    return bits;
}

template <typename T>
__global__ void __launch_bounds__(256) gn_silu_fwd_kernel(const GnArgs a) {
    constexpr int EPL = DT<T>::EPL;
    const int C = a.c1 + a.c2, gs = C / a.G, PPV = C / EPL, P1 = a.c1 / EPL;
    const int n = blockIdx.x / a.blocks_per_n, bn = blockIdx.x % a.blocks_per_n;
    const int64_t npieces = a.V * PPV;
    const int64_t stride = (int64_t)a.blocks_per_n * 256;       // multiple of PPV (blocks_per_sample)
    const float cnt = (float)a.V * gs;
    const T* x1 = reinterpret_cast<const T*>(a.x1) + (size_t)n * a.V * a.c1;
    const T* x2 = a.x2 ? reinterpret_cast<const T*>(a.x2) + (size_t)n * a.V * a.c2 : nullptr;
    T* y = reinterpret_cast<T*>(a.y) + (size_t)n * a.V * C;
    const bool drop = a.p > 0.f;
    const float inv_keep = drop ? 1.f / (1.f - a.p) : 1.f;
    const uint64_t seed = drop ? mix_seed(a.seed, a.seed_step) : 0;
    const int64_t start = (int64_t)bn * 256 + threadIdx.x;
    const int pc = (int)(start % PPV);                          // fixed piece column of this thread
    // per-channel affine once per BLOCK (thread c evaluates channel c into LDS, every thread reads its EPL channels back) instead of
    // EPL times per thread: two exact divisions + rsqrt per channel were ~300 instructions in front of a loop of 16-32 iterations
    __shared__ float tabA[512], tabB[512];                  // (C <= 512: gn_common_check)
    for (int c = threadIdx.x; c < C; c += 256) {
        float mean, rstd;
        gn_affine(a.stats, n, a.G, c / gs, cnt, a.eps, a.gamma[c], a.beta[c], tabA[c], tabB[c], mean, rstd);
    }
    __syncthreads();
    float A[EPL], B[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        A[j] = tabA[pc * EPL + j];
        B[j] = tabB[pc * EPL + j];
    }
    // (the voxel of piece i advances by a constant per iteration: stride % PPV == 0 - no 64-bit division inside the loop)
    int64_t v = start / PPV;
    const int64_t dv = stride / PPV;
    for (int64_t i = start; i < npieces; i += stride, v += dv) {
        const uint4 raw = pc < P1 ? *reinterpret_cast<const uint4*>(x1 + v * a.c1 + pc * EPL)
                                  : *reinterpret_cast<const uint4*>(x2 + v * a.c2 + (pc - P1) * EPL);
        Piece<T> p;
        p.load(raw);
        const unsigned keepbits = drop ? keep_bits_of_piece<EPL>(seed, (uint64_t)n * npieces + (uint64_t)i, a.p) : 0xffu;
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            float o = p.f[j] * A[j] + B[j];
            if (!a.linear) o = silu_f(o);
            if (drop) o *= ((keepbits >> j) & 1u) ? inv_keep : 0.f;
            p.f[j] = o;
        }
        *reinterpret_cast<uint4*>(y + i * EPL) = p.store();
        if (drop && a.mask) a.mask[(size_t)n * npieces + i] = (unsigned char)keepbits;
    }
}

// d(silu(y))/dy
__device__ __forceinline__ float dsilu(float y) {
    const float s = sigmoid_f(y);
    return s * (1.f + y * (1.f - s));
}

// Un-folded GroupNorm backward (a GroupNorm whose gradient did not come out of Conv.dgrad_gn): dyh = dy * keep * silu'(yhat) as its
// own pass; vdm_channel_dot_sums then gives the per-sample (sum dyh, sum dyh * x) and the fixed-order finalize + apply kernels below
// finish - the same bit-reproducible arithmetic as the folded path (the float-atomic reduce / apply kernels of round 1 are gone).
// Thread owns a fixed piece column (stride % PPV == 0 by construction).  Output: a.dx1 = dyh [n][V][C] (may alias dy).
template <typename T>
__global__ void __launch_bounds__(256) gn_dyh_kernel(const GnArgs a) {
    constexpr int EPL = DT<T>::EPL;
    const int C = a.c1 + a.c2, gs = C / a.G, PPV = C / EPL, P1 = a.c1 / EPL;
    const int n = blockIdx.x / a.blocks_per_n, bn = blockIdx.x % a.blocks_per_n;
    const int64_t npieces = a.V * PPV;
    const int64_t stride = (int64_t)a.blocks_per_n * 256;
    const float cnt = (float)a.V * gs;
    const T* x1 = reinterpret_cast<const T*>(a.x1) + (size_t)n * a.V * a.c1;
    const T* x2 = a.x2 ? reinterpret_cast<const T*>(a.x2) + (size_t)n * a.V * a.c2 : nullptr;
    const T* dy = reinterpret_cast<const T*>(a.dy) + (size_t)n * a.V * C;
    T* dyh = reinterpret_cast<T*>(a.dx1) + (size_t)n * a.V * C;
    const bool drop = a.p > 0.f;
    const float inv_keep = drop ? 1.f / (1.f - a.p) : 1.f;
    const uint64_t seed = drop ? mix_seed(a.seed, a.seed_step) : 0;
    const int64_t start = (int64_t)bn * 256 + threadIdx.x;
    const int pc = (int)(start % PPV);
    // per-channel affine once per BLOCK (thread c evaluates channel c into LDS, every thread reads its EPL channels back) instead of
    // EPL times per thread: two exact divisions + rsqrt per channel were ~300 instructions in front of a loop of 16-32 iterations
    __shared__ float tabA[512], tabB[512];                  // (C <= 512: gn_common_check)
    for (int c = threadIdx.x; c < C; c += 256) {
        float mean, rstd;
        gn_affine(a.stats, n, a.G, c / gs, cnt, a.eps, a.gamma[c], a.beta[c], tabA[c], tabB[c], mean, rstd);
    }
    __syncthreads();
    float A[EPL], B[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        A[j] = tabA[pc * EPL + j];
        B[j] = tabB[pc * EPL + j];
    }
    int64_t v = start / PPV;
    const int64_t dv = stride / PPV;
    for (int64_t i = start; i < npieces; i += stride, v += dv) {
        const uint4 raw = pc < P1 ? *reinterpret_cast<const uint4*>(x1 + v * a.c1 + pc * EPL)
                                  : *reinterpret_cast<const uint4*>(x2 + v * a.c2 + (pc - P1) * EPL);
        Piece<T> px, pd;
        px.load(raw);
        pd.load(*reinterpret_cast<const uint4*>(dy + i * EPL));
        const unsigned keepbits = drop ? keep_bits_of_piece<EPL>(seed, (uint64_t)n * npieces + (uint64_t)i, a.p) : 0xffu;      // (the forward's bits)
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            float d = a.linear ? pd.f[j] : pd.f[j] * dsilu(px.f[j] * A[j] + B[j]);
            if (drop) d *= ((keepbits >> j) & 1u) ? inv_keep : 0.f;
            pd.f[j] = d;
        }
        *reinterpret_cast<uint4*>(dyh + i * EPL) = pd.store();
    }
}

__device__ __forceinline__ bool pc_is_first(const GnArgs& a, int epl, int bid, int tid) {
    const int ppv = (a.c1 + a.c2) / epl;
    const long long start = (long long)(bid % a.blocks_per_n) * 256 + tid;
    return (int)(start % ppv) < a.c1 / epl;
}

// ---------------------------------------------------------------------------------------------
// GroupNorm backward, fused form: the dgrad conv that produced dL/dy already stored dyh = dL/dy * keep * silu'(yhat) and
// reduced per (tile, channel) partial sums of (dyh, dyh * x) in its epilogue (conv_common.h, conv_epilogue_gnb).
// finalize: one block per (sample, group) sums the tiles per channel in a fixed order ->
//   chan[n][c] = {T1, T2};  red[n][g] = {sum_c gamma_c T1_c, sum_c gamma_c T2_c};
//   colsum[n][c] = sum_v dx = rstd * (gamma_c T1_c - V m1 - m2 * rstd * (chsum[n][c] - V mean))   (analytic, optional)
// apply: dx = rstd * (gamma * dyh - m1 - xhat * m2) (+ add), m = red / cnt; block 0 also writes dgamma / dbeta = sum_n chan.
// No float atomics anywhere: the backward pass is bit-reproducible.
// ---------------------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(NT) gn_bwd_finalize_kernel(const float* __restrict__ part, int tiles, int C, int gs, int64_t V,
                                                             const float* __restrict__ stats, const float* __restrict__ gamma,
                                                             float eps, const float* __restrict__ chsum, float* __restrict__ red,
                                                             float* __restrict__ chan, float* __restrict__ colsum,
                                                             long long colsum_stride) {
    const int G = C / gs;
    const int n = blockIdx.x / G, g = blockIdx.x % G;
    const float2* p2 = reinterpret_cast<const float2*>(part) + (size_t)n * tiles * C + (size_t)g * gs;
    const int t = threadIdx.x;
    __shared__ float sm[2][NT];
    __shared__ float gr[2];
    tile_partials_fold<NT>(p2, tiles, C, gs, sm);
    const float cnt = (float)V * gs;
    const float gsum = stats[((size_t)n * G + g) * 2], gsq = stats[((size_t)n * G + g) * 2 + 1];
    const float mean = gsum / cnt;
    const float rstd = rsqrtf(fmaxf(gsq / cnt - mean * mean, 0.f) + eps);
    float T1 = 0.f, T2 = 0.f, gam = 0.f;
    if (t < gs) {
        T1 = sm[0][t]; T2 = sm[1][t];
        T2 = rstd * (T2 - mean * T1);                       // the epilogues sum dyh * x (raw): -> sum dyh * xhat
        gam = gamma[g * gs + t];
        chan[((size_t)n * C + g * gs + t) * 2] = T1;
        chan[((size_t)n * C + g * gs + t) * 2 + 1] = T2;
        sm[0][t] = gam * T1; sm[1][t] = gam * T2;
    }
    __syncthreads();
    if (t < 2) {
        float tot = 0.f;
        for (int j = 0; j < gs; ++j) tot += sm[t][j];
        red[((size_t)n * G + g) * 2 + t] = tot;
        gr[t] = tot;
    }
    if (colsum == nullptr) return;                          // (uniform)
    __syncthreads();
    if (t < gs) {
        const float m1 = gr[0] / cnt, m2 = gr[1] / cnt;
        const float xhsum = rstd * (chsum[(size_t)n * C + g * gs + t] - (float)V * mean);
        colsum[(size_t)n * colsum_stride + g * gs + t] = rstd * (gam * T1 - (float)V * m1 - m2 * xhsum);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) gn_bwd_apply_kernel(const GnArgs a) {
    constexpr int EPL = DT<T>::EPL;
    const int C = a.c1 + a.c2, gs = C / a.G, PPV = C / EPL, P1 = a.c1 / EPL;
    const int n = blockIdx.x / a.blocks_per_n, bn = blockIdx.x % a.blocks_per_n;
    if (blockIdx.x == 0) {                                  // parameter gradients: sum over the samples, fixed order
        for (int c = threadIdx.x; c < C; c += 256) {
            float db = 0.f, dg = 0.f;
            for (int k = 0; k < a.n; ++k) { db += a.chan[((size_t)k * C + c) * 2]; dg += a.chan[((size_t)k * C + c) * 2 + 1]; }
            a.dbeta[c] = db;
            a.dgamma[c] = dg;
        }
    }
    const int64_t npieces = a.V * PPV;
    const int64_t stride = (int64_t)a.blocks_per_n * 256;
    const float cnt = (float)a.V * gs;
    const T* x1 = reinterpret_cast<const T*>(a.x1) + (size_t)n * a.V * a.c1;
    const T* x2 = a.x2 ? reinterpret_cast<const T*>(a.x2) + (size_t)n * a.V * a.c2 : nullptr;
    const T* dy = reinterpret_cast<const T*>(a.dy) + (size_t)n * a.V * C;          // dyh
    const T* add1 = a.add1 ? reinterpret_cast<const T*>(a.add1) + (size_t)n * a.V * a.c1 : nullptr;
    const T* add2 = a.add2 ? reinterpret_cast<const T*>(a.add2) + (size_t)n * a.V * a.c2 : nullptr;
    const T* addp = pc_is_first(a, DT<T>::EPL, blockIdx.x, threadIdx.x) ? add1 : add2;
    T* dx1 = reinterpret_cast<T*>(a.dx1) + (size_t)n * a.V * a.c1;
    T* dx2 = a.dx2 ? reinterpret_cast<T*>(a.dx2) + (size_t)n * a.V * a.c2 : nullptr;
    const int64_t start = (int64_t)bn * 256 + threadIdx.x;
    const int pc = (int)(start % PPV);
    // dx = dyh * P + x * Q + R   with  P = rstd gamma, Q = -rstd^2 m2, R = rstd (mean rstd m2 - m1)
    __shared__ float tabP[512], tabQ[512], tabR[512];       // once per block (see gn_silu_fwd_kernel)
    for (int c = threadIdx.x; c < C; c += 256) {
        const int g = c / gs;
        float A, B, mean, rstd;
        const float gam = a.gamma[c];
        gn_affine(a.stats, n, a.G, g, cnt, a.eps, gam, 0.f, A, B, mean, rstd);
        const float m1 = a.red[((size_t)n * a.G + g) * 2] / cnt, m2 = a.red[((size_t)n * a.G + g) * 2 + 1] / cnt;
        tabP[c] = A;
        tabQ[c] = -rstd * rstd * m2;
        tabR[c] = rstd * (mean * rstd * m2 - m1);
    }
    __syncthreads();
    float Pc[EPL], Qc[EPL], Rc[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        Pc[j] = tabP[pc * EPL + j];
        Qc[j] = tabQ[pc * EPL + j];
        Rc[j] = tabR[pc * EPL + j];
    }
    int64_t v = start / PPV;
    const int64_t dv = stride / PPV;
    for (int64_t i = start; i < npieces; i += stride, v += dv) {
        const uint4 raw = pc < P1 ? *reinterpret_cast<const uint4*>(x1 + v * a.c1 + pc * EPL)
                                  : *reinterpret_cast<const uint4*>(x2 + v * a.c2 + (pc - P1) * EPL);
        Piece<T> px, pd, pa;
        px.load(raw);
        pd.load(*reinterpret_cast<const uint4*>(dy + i * EPL));
        if (addp) pa.load(pc < P1 ? *reinterpret_cast<const uint4*>(addp + v * a.c1 + pc * EPL)
                                  : *reinterpret_cast<const uint4*>(addp + v * a.c2 + (pc - P1) * EPL));
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            float o = fmaf(pd.f[j], Pc[j], fmaf(px.f[j], Qc[j], Rc[j]));
            if (addp) o += pa.f[j];
            px.f[j] = o;
        }
        if (pc < P1)
            *reinterpret_cast<uint4*>(dx1 + v * a.c1 + pc * EPL) = px.store();
        else
            *reinterpret_cast<uint4*>(dx2 + v * a.c2 + (pc - P1) * EPL) = px.store();
    }
}

template <typename T>
__global__ void __launch_bounds__(256) pack_input_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t nvox,
                                                        int cpad, T* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * 256) {
        T* o = out + i * cpad;
        st_elem<T>(o, a[i]);
        st_elem<T>(o + 1, b ? b[i] : 0.f);
        for (int j = 2; j < cpad; ++j) st_elem<T>(o + j, 0.f);
    }
}

// ---------------------------------------------------------------------------------------------
// VDM kernels
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) diffuse_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                     const float* __restrict__ alpha, const float* __restrict__ sigma, int64_t per,
                                                     float* __restrict__ z, int blocks_per_n) {
    const int n = blockIdx.x / blocks_per_n, bn = blockIdx.x % blocks_per_n;
    const float al = alpha[n], si = sigma[n];
    const int64_t n4 = per >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + (size_t)n * per);
    const float4* e4 = reinterpret_cast<const float4*>(eps + (size_t)n * per);
    float4* z4 = reinterpret_cast<float4*>(z + (size_t)n * per);
    for (int64_t i = (int64_t)bn * 256 + threadIdx.x; i < n4; i += (int64_t)blocks_per_n * 256) {
        const float4 a = x4[i], b = e4[i];
        z4[i] = make_float4(al * a.x + si * b.x, al * a.y + si * b.y, al * a.z + si * b.z, al * a.w + si * b.w);
    }
    if (bn == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < per; i += 256)
            z[(size_t)n * per + i] = al * x[(size_t)n * per + i] + si * eps[(size_t)n * per + i];
}

// per-block partial sums -> part[(n * blocks_per_n + bn) * 3 + k]; loss_terms_finalize_kernel folds them in a fixed order
// (no float atomics: the loss is bit-reproducible).
__global__ void __launch_bounds__(256) loss_terms_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                        const float* __restrict__ eh, const float* __restrict__ eps0, float s0a0,
                                                        const float* __restrict__ coef, int64_t per, float* __restrict__ part,
                                                        float* __restrict__ deh, int blocks_per_n) {
    const int n = blockIdx.x / blocks_per_n, bn = blockIdx.x % blocks_per_n;
    const float cf = coef[n];
    const size_t base = (size_t)n * per;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int64_t i = (int64_t)bn * 256 + threadIdx.x; i < per; i += (int64_t)blocks_per_n * 256) {
        const float xv = x[base + i], e = eps[base + i], h = eh[base + i];
        const float d = h - e;
        acc[0] += d * d;
        acc[1] += xv * xv;
        const float r = s0a0 * eps0[base + i];       // z0/alpha0 - x
        acc[2] += r * r;
        deh[base + i] = cf * d;
    }
    __shared__ float sm[12];
    block_sum<3>(acc, sm);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.x * 3 + 0] = acc[0];
        part[(size_t)blockIdx.x * 3 + 1] = acc[1];
        part[(size_t)blockIdx.x * 3 + 2] = acc[2];
    }
}

// out[i] (+)= sum_b part[(i / width * blocks + b) * width + i % width]: fixed-order fold of per-block partials.  One block per
// output: thread t sums the partials t, t + 256, ..., then a fixed LDS tree (deterministic).
__global__ void __launch_bounds__(256) fold_partials_kernel(const float* __restrict__ part, int blocks, int width, float* __restrict__ out,
                                                           int accumulate) {
    const int i = blockIdx.x;
    const float* p = part + (size_t)(i / width) * blocks * width + i % width;
    float s = 0.f;
    for (int b = threadIdx.x; b < blocks; b += 256) s += p[(size_t)b * width];
    __shared__ float sm[256];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[i] = accumulate ? out[i] + sm[0] : sm[0];
}

__global__ void __launch_bounds__(256) randn_kernel(float* __restrict__ out, int64_t n, uint64_t seed0, uint64_t sid, const int32_t* __restrict__ seed_step) {
    const uint64_t seed = mix_seed(seed0, seed_step);
    const int64_t n4 = (n + 3) >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 r = randn4(seed, sid, (uint64_t)i);
        const float v[4] = {r.x, r.y, r.z, r.w};
        for (int j = 0; j < 4; ++j)
            if (i * 4 + j < n) out[i * 4 + j] = v[j];
    }
}

// ---------------------------------------------------------------------------------------------
// Head of the network: the NDHWC input of conv_in {z, c_0 .. c_{K-1}, 0 ...} in the compute dtype, written in the pass that makes z -
// ONE 16-byte piece per voxel in both storage types (1 + K <= 4, K = 0 .. 3 conditioning planes).  One skeleton, head_kernel, and four
// sources of what a thread owns (4 consecutive voxels: the four values zz of channel 0 and cc of the K planes):
//   PlainSrc    vdm_pack_fields                            z and cond [n][K][per] as they are (ABI v18)
//   DiffuseSrc  vdm_diffuse_pack, vdm_diffuse_pack_fields  z_t = alpha[n] x + sigma[n] eps, the bits of diffuse_kernel (ABI v11, v18)
//   FlowSrc     vdm_sfm_head                               x_t = (1 - t[n]) x0 + t[n] x1 (+ sigma eps), the plane cond ? x0 : 0 (ABI v21)
//   DiffuseKeepSrc  vdm_diffuse_pack_fields_keep           DiffuseSrc with a per-row keep of the K planes: +0 for a dropped row (ABI v21)
// eps is drawn IN the kernel (Philox, the counters of randn_kernel: same (seed, stream id, element group) -> the same field vdm_randn
// would have written) or read (supplied noise: parity tests).  z is also written as fp32 where it is asked for: randn + diffuse +
// pack_input in one pass over x.  The 16-byte pieces of the packed tensor are re-dealt inside the wave so that every store instruction
// writes 1 KiB contiguously (lane L stores piece 64 r + L of the wave's 256 in round r).
// ---------------------------------------------------------------------------------------------
template <typename T, int K>
__device__ __forceinline__ void deal_pieces(const float (&zz)[4], const float (&cc)[K > 0 ? K : 1][4], int lane, int64_t wave_g0, int64_t per,
                                            T* __restrict__ packed_n) {
    constexpr int EPL = DT<T>::EPL;
    static_assert(K >= 0 && 1 + K <= EPL && 1 + K <= 4, "one 16-byte piece per voxel");
    const int src0 = lane >> 2, comp = lane & 3;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int src = 16 * r + src0;
        float zr = 0.f, cr[K > 0 ? K : 1];
#pragma unroll
        for (int f = 0; f < K; ++f) cr[f] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = __shfl(zz[k], src, 64);
            if (k == comp) zr = a;
#pragma unroll
            for (int f = 0; f < K; ++f) {
                const float b = __shfl(cc[f][k], src, 64);
                if (k == comp) cr[f] = b;
            }
        }
        const int64_t vox = 4 * wave_g0 + 64 * r + lane;            // voxel inside the sample
        if (vox < per) {
            Piece<T> pc;
#pragma unroll
            for (int j = 0; j < EPL; ++j) pc.f[j] = 0.f;
            pc.f[0] = zr;
#pragma unroll
            for (int f = 0; f < K; ++f) pc.f[1 + f] = cr[f];
            *reinterpret_cast<uint4*>(packed_n + (size_t)vox * EPL) = pc.store();
        }
    }
}

// src (by value: a block's own copy) is moved to sample n by seek, then load gives zz and cc of float4 group ic of that sample.
template <typename T, int K, typename Src>
__global__ void __launch_bounds__(256) head_kernel(Src src, int64_t per, float* __restrict__ z, T* __restrict__ packed, int blocks_per_n) {
    constexpr int EPL = DT<T>::EPL;
    const int n = blockIdx.x / blocks_per_n, bn = blockIdx.x % blocks_per_n;
    const int64_t n4 = per >> 2;                                   // (host: per % 4 == 0)
    const size_t base = (size_t)n * per;
    src.template seek<K>(n, per);
    float4* z4 = z ? reinterpret_cast<float4*>(z + base) : nullptr;
    const int lane = threadIdx.x & 63;
    const int64_t rounds = (n4 + (int64_t)blocks_per_n * 256 - 1) / ((int64_t)blocks_per_n * 256);      // uniform trip count: the
    for (int64_t it = 0; it < rounds; ++it) {                                                           // shuffles need every lane
        const int64_t i = (it * blocks_per_n + bn) * 256 + threadIdx.x;
        const bool ok = i < n4;
        const int64_t ic = ok ? i : n4 - 1;                          // (nothing is read outside the inputs)
        float zz[4], cc[K > 0 ? K : 1][4];
        src.template load<K>(n4, ic, zz, cc);
        if (z4 && ok) z4[i] = make_float4(zz[0], zz[1], zz[2], zz[3]);
        deal_pieces<T, K>(zz, cc, lane, i - lane, per, packed + base * EPL);
    }
}

__device__ __forceinline__ void ld4(const float* p, int64_t i, float (&v)[4]) {
    const float4 q = reinterpret_cast<const float4*>(p)[i];
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}

template <int K>
__device__ __forceinline__ void ld_planes(const float* cond_n, int64_t n4, int64_t ic, float (&cc)[K > 0 ? K : 1][4]) {
#pragma unroll
    for (int f = 0; f < K; ++f) ld4(cond_n, (int64_t)f * n4 + ic, cc[f]);
}

// eps of group ic of a sample whose first group is g0 in the batch: read, or drawn when eps_n is NULL
__device__ __forceinline__ void ld_eps(const float* eps_n, uint64_t seed, uint64_t sid, uint64_t g0, int64_t ic, float (&e)[4]) {
    if (eps_n) {
        ld4(eps_n, ic, e);
    } else {
        const float4 r = randn4(seed, sid, g0 + (uint64_t)ic);
        e[0] = r.x; e[1] = r.y; e[2] = r.z; e[3] = r.w;
    }
}

// al * x + si * e as -ffp-contract=fast contracts it in diffuse_kernel: the first product is fused, the second rounded
__device__ __forceinline__ float diffuse_fma(float al, float x, float si, float e) { return fmaf(al, x, uncontracted_mul(si, e)); }

struct PlainSrc {
    static constexpr int KMIN = 1, KMAX = 3;
    const float *z, *cond;
    template <int K>
    __device__ __forceinline__ void seek(int n, int64_t per) {
        z += (size_t)n * per;
        cond += (size_t)n * K * per;
    }
    template <int K>
    __device__ __forceinline__ void load(int64_t n4, int64_t ic, float (&zz)[4], float (&cc)[K > 0 ? K : 1][4]) const {
        ld4(z, ic, zz);
        ld_planes<K>(cond, n4, ic, cc);
    }
};

struct DiffuseSrc {
    static constexpr int KMIN = 0, KMAX = 3;
    const float *x, *cond, *eps;                                    // cond: unused at K = 0; eps: NULL = drawn
    uint64_t seed, sid;
    const int32_t* seed_step;
    const float *alpha, *sigma;
    float al, si;                                                   // of the sample (seek)
    uint64_t g0;
    template <int K>
    __device__ __forceinline__ void seek(int n, int64_t per) {
        const size_t base = (size_t)n * per;
        x += base;
        if (K > 0) cond += base * K;
        if (eps) eps += base;
        seed = mix_seed(seed, seed_step);
        al = alpha[n]; si = sigma[n];
        g0 = (uint64_t)((int64_t)n * (per >> 2));
    }
    template <int K>
    __device__ __forceinline__ void load(int64_t n4, int64_t ic, float (&zz)[4], float (&cc)[K > 0 ? K : 1][4]) const {
        float xv[4], ev[4];
        ld4(x, ic, xv);
        ld_eps(eps, seed, sid, g0, ic, ev);
#pragma unroll
        for (int j = 0; j < 4; ++j) zz[j] = diffuse_fma(al, xv[j], si, ev[j]);
        ld_planes<K>(cond, n4, ic, cc);
    }
};

// DiffuseSrc with a per-row keep of the conditioning planes (vdm_diffuse_pack_fields_keep: conditioning dropout of classifier-free
// guidance training).  keep_s[n] is read once in seek; a block serves one sample, so the branch in load is uniform.  A dropped row
// writes +0 into planes 1 .. K and never reads its cond planes; z_t / channel 0 are DiffuseSrc's.  keep_s NULL: every row kept.
// A source type of its own: the instantiations of head_kernel<.., DiffuseSrc> behind the older entries are not touched.
struct DiffuseKeepSrc {
    static constexpr int KMIN = 1, KMAX = 3;
    DiffuseSrc d;
    const float* keep_s;
    bool kept;                                                      // of the sample (seek)
    template <int K>
    __device__ __forceinline__ void seek(int n, int64_t per) {
        d.template seek<K>(n, per);
        kept = keep_s ? keep_s[n] != 0.f : true;
    }
    template <int K>
    __device__ __forceinline__ void load(int64_t n4, int64_t ic, float (&zz)[4], float (&cc)[K > 0 ? K : 1][4]) const {
        float nocond[1][4];
        d.template load<0>(n4, ic, zz, nocond);
        if (kept) {
            ld_planes<K>(d.cond, n4, ic, cc);
        } else {
#pragma unroll
            for (int f = 0; f < K; ++f)
#pragma unroll
                for (int j = 0; j < 4; ++j) cc[f][j] = 0.f;
        }
    }
};

// ---------------------------------------------------------------------------------------------
// Conditioning dropout of classifier-free guidance training (ABI v21): the per-row keep draw and the row select.
//   cond_keep : keep[r] = unit(word 0 of Philox(key = mix_seed(seed, step), counter = (row lo, row hi, 0xCFD0, 0))) > p ? 1 : 0 with
//               row = row0 + r the GLOBAL row (rank * B + i) - the rule of the fp32 dropout byte: p = 0 keeps all, p = 1 drops all
//   mask_rows : out[r][j] = keep[r] != 0 ? v[r][j] : +0 - a select, not a product: NaN / Inf of a dropped row do not get through
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cond_keep_kernel(float p, uint64_t seed0, const int32_t* __restrict__ seed_step, uint64_t row0,
                                                       int64_t rows, float* __restrict__ keep) {
    const uint64_t seed = mix_seed(seed0, seed_step);
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
        const uint64_t row = row0 + (uint64_t)r;
        uint32_t rnd[4];
        Philox::gen((uint32_t)row, (uint32_t)(row >> 32), 0xCFD0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), rnd);
        keep[r] = u32_to_unit(rnd[0]) > p ? 1.f : 0.f;
    }
}

// grid (x blocks, row blocks): a block works on one row at a time, so the select is uniform (a dropped row is never read).  vec: both
// pointers 16-byte aligned and dim % 4 == 0.  out may be v (no __restrict__ on the two): every element is read and written by one thread.
__global__ void __launch_bounds__(256) mask_rows_kernel(const float* v, const float* __restrict__ keep, int64_t rows, int64_t dim, int vec,
                                                       float* out) {
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const bool kept = keep[r] != 0.f;
        const float* vr = v + (size_t)r * dim;
        float* o = out + (size_t)r * dim;
        if (vec) {
            const int64_t d4 = dim >> 2;
            for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < d4; i += (int64_t)gridDim.x * 256)
                reinterpret_cast<float4*>(o)[i] = kept ? reinterpret_cast<const float4*>(vr)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < dim; i += (int64_t)gridDim.x * 256) o[i] = kept ? vr[i] : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Flow matching (ABI v21): the head and the loss of an SFM training step.  Their arithmetic is pinned, bit for bit, to the chain of
// generic launches they replace; the roundings are spelled out (fmaf / uncontracted_mul) as -ffp-contract=fast contracts the older
// kernels' expressions, so that equality does not rest on two copies of one source line being contracted alike.
//   sfm_interp : diffuse_kernel's al * x + si * e for (x = x1, e = x0, al = t, si = 1 - t) = fma(t, x1, (1 - t) * x0), then the same
//                expression for (x = x_t, e = eps, al = 1, si = sigma) = x_t + sigma * eps (product rounded, then one add)
//   sfm_sq4    : loss_terms_rng_kernel's (d0 d0 + d1 d1) + (d2 d2 + d3 d3) = fma(d0, d0, d1 * d1) + fma(d2, d2, d3 * d3)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sfm_interp(float t, float omt, float x0, float x1, bool noisy, float sigma, float e) {
    const float xt = diffuse_fma(t, x1, omt, x0);
    return noisy ? xt + uncontracted_mul(sigma, e) : xt;
}

__device__ __forceinline__ float sfm_sq4(float d0, float d1, float d2, float d3) {
    return fmaf(d0, d0, uncontracted_mul(d1, d1)) + fmaf(d2, d2, uncontracted_mul(d3, d3));
}

// Head source: x_t = (1 - t[n]) x0 + t[n] x1 (+ sigma eps) and the plane cond ? x0 : 0 - diffuse + (randn + diffuse) + pack_input in
// one pass.  sigma == 0 (uniform), or eps supplied: neither the generator nor seed_step is touched.
struct FlowSrc {
    static constexpr int KMIN = 1, KMAX = 1;
    const float *x0, *x1, *eps;
    uint64_t seed, sid;
    const int32_t* seed_step;
    const float* t;
    float sigma;
    int cond;
    float tn, omt;                                                  // of the sample (seek)
    uint64_t g0;
    template <int K>
    __device__ __forceinline__ void seek(int n, int64_t per) {
        const size_t base = (size_t)n * per;
        x0 += base; x1 += base;
        const bool noisy = sigma > 0.f;
        seed = noisy && !eps ? mix_seed(seed, seed_step) : 0;
        eps = noisy && eps ? eps + base : nullptr;
        tn = t[n]; omt = 1.0f - tn;                                 // (1 - t rounded to fp32 first, as the chain's host expression)
        g0 = (uint64_t)((int64_t)n * (per >> 2));
    }
    template <int K>
    __device__ __forceinline__ void load(int64_t n4, int64_t ic, float (&zz)[4], float (&cc)[1][4]) const {
        static_assert(K == 1, "one plane: x0 or +0");
        const bool noisy = sigma > 0.f;
        float av[4], bv[4], ev[4] = {0.f, 0.f, 0.f, 0.f};
        ld4(x0, ic, av);
        ld4(x1, ic, bv);
        if (noisy) ld_eps(eps, seed, sid, g0, ic, ev);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            zz[j] = sfm_interp(tn, omt, av[j], bv[j], noisy, sigma, ev[j]);
            cc[0][j] = cond ? av[j] : 0.f;
        }
    }
};

// Loss: part[block] = sum (v_hat - (x1 - x0))^2 and d_v = coef[n] (v_hat - (x1 - x0)); the target field is never written.  The residual,
// the per-thread accumulation and the block fold are those of loss_terms_rng_kernel's first sum on the materialised target (x1 - x0 is
// what diffuse_kernel gives for alpha = 1, sigma = -1: one rounded subtraction).
__global__ void __launch_bounds__(256) sfm_loss_kernel(const float* __restrict__ vh, const float* __restrict__ x0, const float* __restrict__ x1,
                                                      const float* __restrict__ coef, int64_t per, float* __restrict__ part,
                                                      float* __restrict__ dv, int blocks_per_n) {
    const int n = blockIdx.x / blocks_per_n, bn = blockIdx.x % blocks_per_n;
    const float cf = coef[n];
    const size_t base = (size_t)n * per;
    const int64_t n4 = per >> 2;
    const float4* h4 = reinterpret_cast<const float4*>(vh + base);
    const float4* a4 = reinterpret_cast<const float4*>(x0 + base);
    const float4* b4 = reinterpret_cast<const float4*>(x1 + base);
    float4* d4 = reinterpret_cast<float4*>(dv + base);
    float acc[1] = {0.f};
    for (int64_t i = (int64_t)bn * 256 + threadIdx.x; i < n4; i += (int64_t)blocks_per_n * 256) {
        const float4 hv = h4[i], av = a4[i], bv = b4[i];
        const float d0 = hv.x - (bv.x - av.x), d1 = hv.y - (bv.y - av.y), d2 = hv.z - (bv.z - av.z), d3 = hv.w - (bv.w - av.w);
        acc[0] += sfm_sq4(d0, d1, d2, d3);
        d4[i] = make_float4(cf * d0, cf * d1, cf * d2, cf * d3);
    }
    __shared__ float sm[4];
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

// K8 with the noise fields regenerated from their Philox counters instead of read (eps / eps0 NULL): the two 4-byte-per-element
// fields of a training step never exist in memory.  Vector form of loss_terms_kernel (4 elements per thread; per % 4 == 0).
__global__ void __launch_bounds__(256) loss_terms_rng_kernel(const float* __restrict__ x, const float* __restrict__ eps, uint64_t seed_e0,
                                                            uint64_t sid_e, const float* __restrict__ eh, const float* __restrict__ eps0,
                                                            uint64_t seed_00, uint64_t sid_0, const int32_t* __restrict__ seed_step, float s0a0,
                                                            const float* __restrict__ coef, int64_t per, float* __restrict__ part,
                                                            float* __restrict__ deh, int blocks_per_n) {
    const int n = blockIdx.x / blocks_per_n, bn = blockIdx.x % blocks_per_n;
    const float cf = coef[n];
    const size_t base = (size_t)n * per;
    const int64_t n4 = per >> 2;
    const uint64_t seed_e = mix_seed(seed_e0, seed_step), seed_0 = mix_seed(seed_00, seed_step);
    const float4* x4 = reinterpret_cast<const float4*>(x + base);
    const float4* h4 = reinterpret_cast<const float4*>(eh + base);
    const float4* e4 = eps ? reinterpret_cast<const float4*>(eps + base) : nullptr;
    const float4* o4 = eps0 ? reinterpret_cast<const float4*>(eps0 + base) : nullptr;
    float4* d4 = reinterpret_cast<float4*>(deh + base);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int64_t i = (int64_t)bn * 256 + threadIdx.x; i < n4; i += (int64_t)blocks_per_n * 256) {
        const uint64_t g = (uint64_t)((int64_t)n * n4 + i);
        const float4 xv = x4[i], hv = h4[i];
        const float4 ev = e4 ? e4[i] : randn4(seed_e, sid_e, g);
        const float4 ov = o4 ? o4[i] : randn4(seed_0, sid_0, g);
        const float d0 = hv.x - ev.x, d1 = hv.y - ev.y, d2 = hv.z - ev.z, d3 = hv.w - ev.w;
        acc[0] += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        acc[1] += (xv.x * xv.x + xv.y * xv.y) + (xv.z * xv.z + xv.w * xv.w);
        const float r0 = s0a0 * ov.x, r1 = s0a0 * ov.y, r2 = s0a0 * ov.z, r3 = s0a0 * ov.w;
        acc[2] += (r0 * r0 + r1 * r1) + (r2 * r2 + r3 * r3);
        d4[i] = make_float4(cf * d0, cf * d1, cf * d2, cf * d3);
    }
    __shared__ float sm[12];
    block_sum<3>(acc, sm);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.x * 3 + 0] = acc[0];
        part[(size_t)blockIdx.x * 3 + 1] = acc[1];
        part[(size_t)blockIdx.x * 3 + 2] = acc[2];
    }
}

// K7b: the per-sample sums of the learned schedule's gradient, part[block] = {sum dz x, sum dz eps} (dz = d loss / d z_t); eps read or
// regenerated from the Philox counters of diffuse_pack_kernel (same (seed, stream id, element group) keying: the noise field is never
// stored).  Vector form, 4 elements per thread; fold_partials_kernel sums the partials in a fixed order (bit-reproducible).
__global__ void __launch_bounds__(256) schedule_grad_sums_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                                const float* __restrict__ eps, uint64_t seed0, uint64_t sid,
                                                                const int32_t* __restrict__ seed_step, int64_t per, float* __restrict__ part,
                                                                int blocks_per_n) {
    const int n = blockIdx.x / blocks_per_n, bn = blockIdx.x % blocks_per_n;
    const size_t base = (size_t)n * per;
    const int64_t n4 = per >> 2;
    const uint64_t seed = mix_seed(seed0, seed_step);
    const float4* d4 = reinterpret_cast<const float4*>(dz + base);
    const float4* x4 = reinterpret_cast<const float4*>(x + base);
    const float4* e4 = eps ? reinterpret_cast<const float4*>(eps + base) : nullptr;
    float acc[2] = {0.f, 0.f};
    for (int64_t i = (int64_t)bn * 256 + threadIdx.x; i < n4; i += (int64_t)blocks_per_n * 256) {
        const float4 dv = d4[i], xv = x4[i];
        const float4 ev = e4 ? e4[i] : randn4(seed, sid, (uint64_t)((int64_t)n * n4 + i));
        acc[0] += (dv.x * xv.x + dv.y * xv.y) + (dv.z * xv.z + dv.w * xv.w);
        acc[1] += (dv.x * ev.x + dv.y * ev.y) + (dv.z * ev.z + dv.w * ev.w);
    }
    __shared__ float sm[8];
    block_sum<2>(acc, sm);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.x * 2 + 0] = acc[0];
        part[(size_t)blockIdx.x * 2 + 1] = acc[1];
    }
}

// One element of the ancestral update z <- ratio * (z - cs * e) + scale * noise, shared by ancestral_kernel and ancestral_rows_kernel.
// The rounding is spelled out - fma(-cs, e, z), then the two products rounded and added - which is what ancestral_kernel has always
// compiled to, so the row-keyed kernel gives the same bits whatever the compiler packs.  cfg: classifier-free guidance - the noise
// estimate is (1 + w) * eh - w * eu (conditional / v-masked UNet outputs, the two halves of one batch-doubled forward), blended here so
// that the guided estimate never exists in memory.
__device__ __forceinline__ float ancestral_update(float z, float eh, float eu, bool cfg, float w, float ratio, float cs, float scale,
                                                  float nz) {
    const float e = cfg ? uncontracted_mul(1.f + w, eh) - uncontracted_mul(w, eu) : eh;
    return uncontracted_mul(ratio, fmaf(-cs, e, z)) + uncontracted_mul(scale, nz);
}

__global__ void __launch_bounds__(256) ancestral_kernel(float* __restrict__ z, const float* __restrict__ eh,
                                                       const float* __restrict__ eu, float w,
                                                       const float* __restrict__ noise, const float* __restrict__ coef,
                                                       const int32_t* __restrict__ step_ptr, uint64_t seed, int64_t n) {
    const int step = *step_ptr;
    const float ratio = coef[step * 4 + 0], cs = coef[step * 4 + 1], scale = coef[step * 4 + 2];
    const int64_t n4 = (n + 3) >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float nz[4];
        if (noise) {
            for (int j = 0; j < 4; ++j) nz[j] = (i * 4 + j < n) ? noise[i * 4 + j] : 0.f;
        } else {
            const float4 r = randn4(seed, (uint64_t)(step + 1), (uint64_t)i);
            nz[0] = r.x; nz[1] = r.y; nz[2] = r.z; nz[3] = r.w;
        }
        for (int j = 0; j < 4; ++j) {
            const int64_t k = i * 4 + j;
            if (k < n) z[k] = ancestral_update(z[k], eh[k], eu ? eu[k] : 0.f, eu != nullptr, w, ratio, cs, scale, nz[j]);
        }
    }
}

// Row-keyed form: row r (blockIdx.y) of z [rows][per] draws its noise from (seeds[r], step + 1, float4 group index within the row), so a
// chain's noise does not depend on the batch it is sampled in (rows == 1: the stream of ancestral_kernel with seed = seeds[0]).
// per % 4 == 0 and 16-byte aligned rows (checked by the entry point).
__global__ void __launch_bounds__(256) ancestral_rows_kernel(float* __restrict__ z, const float* __restrict__ eh,
                                                            const float* __restrict__ eu, float w, const float* __restrict__ coef,
                                                            const int32_t* __restrict__ step_ptr, const uint64_t* __restrict__ seeds,
                                                            int64_t per) {
    const int step = *step_ptr;
    const float ratio = coef[step * 4 + 0], cs = coef[step * 4 + 1], scale = coef[step * 4 + 2];
    const uint64_t seed = seeds[blockIdx.y];
    const size_t base = (size_t)blockIdx.y * per;
    const int64_t n4 = per >> 2;
    float4* z4 = reinterpret_cast<float4*>(z + base);
    const float4* h4 = reinterpret_cast<const float4*>(eh + base);
    const float4* u4 = eu ? reinterpret_cast<const float4*>(eu + base) : nullptr;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 r = randn4(seed, (uint64_t)(step + 1), (uint64_t)i);
        const float4 hv = h4[i];
        const float4 uv = u4 ? u4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 zv = z4[i];
        zv.x = ancestral_update(zv.x, hv.x, uv.x, u4 != nullptr, w, ratio, cs, scale, r.x);
        zv.y = ancestral_update(zv.y, hv.y, uv.y, u4 != nullptr, w, ratio, cs, scale, r.y);
        zv.z = ancestral_update(zv.z, hv.z, uv.z, u4 != nullptr, w, ratio, cs, scale, r.z);
        zv.w = ancestral_update(zv.w, hv.w, uv.w, u4 != nullptr, w, ratio, cs, scale, r.w);
        z4[i] = zv;
    }
}

// K9m: one element of the multistep update (DPM-Solver++(2M) on the VDM's data prediction, Adams-Bashforth 2 on the flow-matching
// velocity; a first-order row is DDIM / Euler).  Every rounding is spelled out, so both libraries give the same bits whatever the
// compiler contracts:
//   e   = cfg ? rn(rn(rn(1 + w) * eh) - rn(w * eu)) : eh            (the blend of ancestral_update)
//   est = fma(e_z, z, rn(e_e * e))
//   a   = fma(w_z, z, rn(w_x * est))
//   z'  = hist ? fma(w_p, prev, a) : a
// hist = (w_p != 0), the same for every lane: a row without history (the first step: the buffer is uninitialised and may hold NaN)
// does not load prev at all.
__device__ __forceinline__ float multistep_est(float z, float eh, float eu, bool cfg, float w, float e_z, float e_e) {
    const float e = cfg ? uncontracted_mul(1.f + w, eh) - uncontracted_mul(w, eu) : eh;
    return fmaf(e_z, z, uncontracted_mul(e_e, e));
}

__device__ __forceinline__ float multistep_update(float z, float est, float prev, bool hist, float w_z, float w_x, float w_p) {
    const float a = fmaf(w_z, z, uncontracted_mul(w_x, est));
    return hist ? fmaf(w_p, prev, a) : a;
}

// z <- w_z z + w_x est + w_p prev, prev <- est at the row *step_ptr of coef[steps][8] = {e_z, e_e, w_z, w_x, w_p, t_net, 0, 0}.  The
// first n_vec float4 groups go through 16-byte loads and stores (n_vec = 0 when a field is not 16-byte aligned), the ragged tail
// [4 n_vec, n) element by element.
__global__ void __launch_bounds__(256) multistep_kernel(float* __restrict__ z, const float* __restrict__ eh,
                                                       const float* __restrict__ eu, float w, float* __restrict__ prev,
                                                       const float* __restrict__ coef, const int32_t* __restrict__ step_ptr,
                                                       int64_t n_vec, int64_t n) {
    const float* row = coef + (size_t)(*step_ptr) * 8;
    const float e_z = row[0], e_e = row[1], w_z = row[2], w_x = row[3], w_p = row[4];
    const bool hist = w_p != 0.f, cfg = eu != nullptr;
    float4* z4 = reinterpret_cast<float4*>(z);
    float4* p4 = reinterpret_cast<float4*>(prev);
    const float4* h4 = reinterpret_cast<const float4*>(eh);
    const float4* u4 = reinterpret_cast<const float4*>(eu);
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < n_vec; i += stride) {
        const float4 hv = h4[i];
        const float4 uv = cfg ? u4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 pv = hist ? p4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 zv = z4[i], ev;
        ev.x = multistep_est(zv.x, hv.x, uv.x, cfg, w, e_z, e_e);
        ev.y = multistep_est(zv.y, hv.y, uv.y, cfg, w, e_z, e_e);
        ev.z = multistep_est(zv.z, hv.z, uv.z, cfg, w, e_z, e_e);
        ev.w = multistep_est(zv.w, hv.w, uv.w, cfg, w, e_z, e_e);
        zv.x = multistep_update(zv.x, ev.x, pv.x, hist, w_z, w_x, w_p);
        zv.y = multistep_update(zv.y, ev.y, pv.y, hist, w_z, w_x, w_p);
        zv.z = multistep_update(zv.z, ev.z, pv.z, hist, w_z, w_x, w_p);
        zv.w = multistep_update(zv.w, ev.w, pv.w, hist, w_z, w_x, w_p);
        z4[i] = zv;
        p4[i] = ev;
    }
    for (int64_t k = n_vec * 4 + tid; k < n; k += stride) {
        const float est = multistep_est(z[k], eh[k], cfg ? eu[k] : 0.f, cfg, w, e_z, e_e);
        z[k] = multistep_update(z[k], est, hist ? prev[k] : 0.f, hist, w_z, w_x, w_p);
        prev[k] = est;
    }
}

// out[c] = sum over rows of x[row][c] (bias gradients of the attention block's 1x1 projections); one workgroup per 16-byte piece
// column, fixed summation order
template <typename T>
__global__ void __launch_bounds__(256) channel_sums_kernel(const T* __restrict__ x, int64_t rows, int C, float* __restrict__ out) {
    constexpr int EPL = DT<T>::EPL;
    __shared__ float sm[4 * EPL];
    float acc[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) acc[j] = 0.f;
    for (int64_t r = threadIdx.x; r < rows; r += 256) {
        Piece<T> p;
        p.load(*reinterpret_cast<const uint4*>(x + r * C + blockIdx.x * EPL));
#pragma unroll
        for (int j = 0; j < EPL; ++j) acc[j] += p.f[j];
    }
    block_sum<EPL>(acc, sm);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < EPL; ++j) out[blockIdx.x * EPL + j] = acc[j];
    }
}

// out[n][c][2] = (sum_rows a, sum_rows a * b) per sample, b = concat(b1 [c1 ch], b2 [c2 ch]): the (sum dyh, sum dyh * x) channel totals
// that vdm_gn_bwd_finalize takes as "one tile per sample" partials - the deterministic GroupNorm backward of a norm whose gradient did
// not come out of a dgrad epilogue.  One workgroup per (16-byte piece column, sample), fixed summation order.
template <typename T>
__global__ void __launch_bounds__(256) channel_dot_sums_kernel(const T* __restrict__ a, const T* __restrict__ b1, int c1,
                                                               const T* __restrict__ b2, int c2, int64_t rows, float* __restrict__ out) {
    constexpr int EPL = DT<T>::EPL;
    __shared__ float sm[4 * 2 * EPL];
    const int n = blockIdx.y, C = c1 + c2, col = blockIdx.x * EPL;
    const T* an = a + (size_t)n * rows * C + col;
    const bool first = col < c1;
    const T* bn = first ? b1 + (size_t)n * rows * c1 + col : b2 + (size_t)n * rows * c2 + (col - c1);
    const int cb = first ? c1 : c2;
    float acc[2 * EPL];
#pragma unroll
    for (int j = 0; j < 2 * EPL; ++j) acc[j] = 0.f;
    for (int64_t r = threadIdx.x; r < rows; r += 256) {
        Piece<T> pa, pb;
        pa.load(*reinterpret_cast<const uint4*>(an + r * C));
        pb.load(*reinterpret_cast<const uint4*>(bn + r * cb));
#pragma unroll
        for (int j = 0; j < EPL; ++j) { acc[2 * j] += pa.f[j]; acc[2 * j + 1] = fmaf(pa.f[j], pb.f[j], acc[2 * j + 1]); }
    }
    block_sum<2 * EPL>(acc, sm);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < 2 * EPL; ++j) out[((size_t)n * C + col) * 2 + j] = acc[j];
    }
}

__global__ void step_inc_kernel(int32_t* p) { *p += 1; }

// ---------------------------------------------------------------------------------------------
// The scalar glue of a VDM training step as three tiny kernels (it used to be ~60 ATen launches of 5 us each, all on the critical
// path: time grid, alpha / sigma, the ELBO terms, the clip coefficient).
// train_scalars: out[5][B] = {t, alpha_t, sigma_t, coef = gamma'(t) * bpd / B, t_norm} for the fixed linear schedule [D9, D10];
//   t_i = (u0 + (rank * B + i) / (world * B)) mod 1 (antithetic stratification over the global batch) when u0 != NULL, else times[i].
__global__ void train_scalars_kernel(const float* __restrict__ u0, const float* __restrict__ times, int B, int rank, int world,
                                     float gamma_min, float gamma_max, float bpd_over_B, float* __restrict__ out, uint64_t seed,
                                     const int32_t* __restrict__ seed_step) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    float t;
    if (u0 || !times) {
        float u;
        if (u0) {
            u = u0[0];
        } else {                                               // one uniform draw per step from (seed, device step counter): same on every rank
            uint32_t r[4];
            const uint64_t sd = mix_seed(seed, seed_step);
            Philox::gen(0u, 0u, 0x71e5u, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), r);
            u = u32_to_unit(r[0]);
        }
        t = u + (float)(rank * B + i) / (float)(world * B);
        t -= floorf(t);                                        // torch.remainder(., 1.0)
    } else {
        t = times[i];
    }
    const float g = gamma_min + (gamma_max - gamma_min) * t;
    out[i] = t;
    out[B + i] = sqrtf(1.0f / (1.0f + expf(g)));              // alpha = sqrt(sigmoid(-gamma))
    out[2 * B + i] = sqrtf(1.0f / (1.0f + expf(-g)));         // sigma = sqrt(sigmoid(gamma))
    out[3 * B + i] = (gamma_max - gamma_min) * bpd_over_B;    // 2 w_n, w_n = 0.5 gamma'(t) bpd / B
    out[4 * B + i] = (g - gamma_min) / (gamma_max - gamma_min);
}

// elbo_assemble: out[4] = {elbo, diffusion, latent, reconstruction} (bits/dim, batch means) from the per-sample sums of
// vdm_loss_terms: diffusion = 0.5 sum_n coef_n S0_n;  latent = mean_n (c_lat0 + c_lat1 S1_n);  recons = mean_n (c_rec0 S2_n + c_rec1)
// (the constants fold numel, var_1, data_noise and bits-per-dim; computed in fp64 on the host).  One wave, fixed order.
__global__ void elbo_assemble_kernel(const float* __restrict__ sums, const float* __restrict__ coef, int B, float c_lat0, float c_lat1,
                                     float c_rec0, float c_rec1, float* __restrict__ out) {
    if (threadIdx.x != 0) return;
    float diff = 0.f, lat = 0.f, rec = 0.f;
    for (int n = 0; n < B; ++n) {
        diff += 0.5f * coef[n] * sums[3 * n];
        lat += c_lat0 + c_lat1 * sums[3 * n + 1];
        rec += c_rec0 * sums[3 * n + 2] + c_rec1;
    }
    lat /= (float)B; rec /= (float)B;
    out[0] = diff + lat + rec; out[1] = diff; out[2] = lat; out[3] = rec;
}

// clip_scale: x *= min(1, max_norm / (sqrt(sumsq) + 1e-6)) - the global-norm clip [D11, gradient_clip_val] with the coefficient
// computed from the device-side sum of squares inside the scaling pass (no host sync, no separate coefficient kernels).
__global__ void __launch_bounds__(256) clip_scale_kernel(float* __restrict__ x, int64_t n, const float* __restrict__ sumsq, float max_norm) {
    const float coef = fminf(max_norm / (sqrtf(sumsq[0]) + 1.0e-6f), 1.0f);
    if (coef == 1.0f) return;                                  // (uniform) nothing to do below the threshold
    const int64_t n4 = n >> 2;
    float4* x4 = reinterpret_cast<float4*>(x);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 v = x4[i];
        v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
        x4[i] = v;
    }
    if (blockIdx.x == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) x[i] *= coef;
}

__global__ void __launch_bounds__(256) sumsq_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ part) {
    float acc[1] = {0.f};
    const int64_t n4 = n >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = x4[i];
        acc[0] += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    if (blockIdx.x == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) acc[0] += x[i] * x[i];
    __shared__ float sm[4];
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

// blocks*256 must be a multiple of pieces-per-voxel (fixed piece column per thread): ppv = C/EPL is a power of two times {1,3,5},
// so the block count is a multiple of m = ppv/gcd(ppv,256)
static int piece_multiple(int ppv) {
    int g = ppv, b = 256;
    while (b) { const int t = g % b; g = b; b = t; }
    return ppv / g;
}

// blocks per sample of the streaming kernels (gn_silu_fwd, gn_dyh, gn_bwd_apply): ~8 pieces per thread, about 2048 blocks in all,
// rounded UP to a multiple of m (these kernels own no workspace: a few blocks over 2048 are harmless)
static int blocks_per_sample(int64_t npieces, int ppv, int n) {
    int64_t want = (npieces + 256 * 8 - 1) / (256 * 8);          // ~8 pieces per thread
    int64_t cap = 2048 / (n > 0 ? n : 1);
    if (cap < 1) cap = 1;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    const int m = piece_multiple(ppv);
    want = (want + m - 1) / m * m;
    return (int)want;
}

// the same for the full statistics pass, whose n * blocks rows of partials must fit the workspace of vdm_gn_stats (2048 rows at 64
// groups): where the rounding crossed the cap, back down to the last multiple of m under it - never below m itself (vdm_gn_stats
// refuses the call whose n * m rows do not fit).  Equal to blocks_per_sample wherever that stayed within the cap (m = 1: always).
static int stats_blocks_per_sample(int64_t npieces, int ppv, int n) {
    int64_t want = blocks_per_sample(npieces, ppv, n);
    const int64_t cap = 2048 / (n > 0 ? n : 1);
    const int m = piece_multiple(ppv);
    if (want > cap) want = cap / m * m;
    if (want < m) want = m;
    return (int)want;
}

}  // namespace vdm

using namespace vdm;

static int gn_common_check(int c1, int c2, int n, int64_t voxels, int groups, int dtype, const char* who) {
    const int epl = dtype == VDM_F32 ? 4 : 8;
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "%s: bad dtype %d", who, dtype);
    VDM_REQUIRE(n > 0 && voxels > 0 && groups > 0 && groups <= 64, "%s: bad n/voxels/groups", who);
    VDM_REQUIRE(c1 > 0 && c2 >= 0 && (c1 % epl) == 0 && (c2 % epl) == 0, "%s: channel counts must be multiples of %d (got %d,%d)", who, epl, c1, c2);
    const int C = c1 + c2;
    VDM_REQUIRE(C % groups == 0 && C <= 512, "%s: channels %d not divisible by groups %d or > 512", who, C, groups);
    VDM_REQUIRE(c1 % (C / groups) == 0, "%s: group straddles the concat boundary", who);
    return VDM_OK;
}

extern "C" int vdm_gn_stats(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups, int dtype, float* stats,
                            float* workspace, const float* part1, int tiles1, const float* part2, int tiles2, float* chsum,
                            void* stream) {
    int e = gn_common_check(c1, c2, n, voxels, groups, dtype, "gn_stats");
    if (e) return e;
    VDM_REQUIRE(stats && workspace && (x1 || part1) && (c2 == 0 || x2 || part2), "gn_stats: NULL pointer");
    VDM_REQUIRE((!part1 || tiles1 > 0) && (!part2 || tiles2 > 0), "gn_stats: partials need a positive tile count");
    VDM_REQUIRE(!chsum || (part1 && (c2 == 0 || part2)), "gn_stats: per-channel sums are produced from conv partials only");
    hipStream_t s = (hipStream_t)stream;
    const int epl = dtype == VDM_F32 ? 4 : 8;
    const int gs = (c1 + c2) / groups;
    const void* xs[2] = {x1, x2};
    const int cs[2] = {c1, c2};
    const float* parts[2] = {part1, part2};
    const int tiles[2] = {tiles1, tiles2};
    // every refusal comes before the first launch: a call either runs whole or leaves stats / chsum / workspace untouched
    for (int k = 0; k < 2; ++k) {
        if (cs[k] == 0) continue;
        if (parts[k]) {                                   // (tile_partials_fold<256>: one thread per channel of the group)
            VDM_REQUIRE(gs <= 256, "gn_stats: %d channels per group from conv partials, the limit is 256", gs);
            continue;
        }
        const int ppv = cs[k] / epl;
        const int64_t rows = (int64_t)n * stats_blocks_per_sample(voxels * ppv, ppv, n);
        VDM_REQUIRE(rows * 2 * groups * (int64_t)sizeof(float) <= (int64_t)VDM_GN_STATS_WS_BYTES,
                    "gn_stats: %lld rows of %d partials exceed the workspace limit VDM_GN_STATS_WS_BYTES = %d bytes", (long long)rows,
                    2 * groups, (int)VDM_GN_STATS_WS_BYTES);
    }
    int g0 = 0;
    if (parts[0] && c2 > 0 && parts[1]) {                  // both halves of a concat come with conv partials: one launch
        hipLaunchKernelGGL(gn_stats_from_partials_kernel<256>, dim3(n * ((c1 + c2) / gs)), dim3(256), 0, s, parts[0], tiles[0], c1, gs, groups, 0, stats,
                           chsum, c1 + c2, 0, parts[1], tiles[1], c2);
        VDM_LAUNCH_CHECK("gn_stats_from_partials_kernel");
        return VDM_OK;
    }
    for (int k = 0; k < 2; ++k) {
        if (cs[k] == 0) continue;
        if (parts[k]) {                                   // statistics already reduced per tile by the producing conv
            hipLaunchKernelGGL(gn_stats_from_partials_kernel<256>, dim3(n * (cs[k] / gs)), dim3(256), 0, s, parts[k], tiles[k], cs[k], gs, groups, g0,
                               stats, chsum, c1 + c2, g0 * gs, (const float*)nullptr, 0, 0);
            VDM_LAUNCH_CHECK("gn_stats_from_partials_kernel");
            g0 += cs[k] / gs;
            continue;
        }
        const int ppv = cs[k] / epl;
        const int bpn = stats_blocks_per_sample(voxels * ppv, ppv, n);
        if (dtype == VDM_F32)
            hipLaunchKernelGGL(gn_stats_kernel<float>, dim3(bpn * n), dim3(256), 0, s, (const float*)xs[k], cs[k], voxels, gs, groups, g0, workspace, bpn);
        else
            hipLaunchKernelGGL(gn_stats_kernel<bf16_t>, dim3(bpn * n), dim3(256), 0, s, (const bf16_t*)xs[k], cs[k], voxels, gs, groups, g0, workspace, bpn);
        hipLaunchKernelGGL(gn_stats_finalize_kernel, dim3(n), dim3(256), 0, s, (const float*)workspace, groups, g0, cs[k] / gs, bpn, stats);
        VDM_LAUNCH_CHECK("gn_stats_kernel");
        g0 += cs[k] / gs;
    }
    return VDM_OK;
}

static GnArgs gn_args(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups, int dtype, const float* stats,
                      const float* gamma, const float* beta, float eps, float p, uint64_t seed) {
    GnArgs a{};
    a.x1 = x1; a.x2 = x2; a.c1 = c1; a.c2 = c2; a.n = n; a.G = groups; a.V = voxels;
    a.stats = stats; a.gamma = gamma; a.beta = beta; a.eps = eps; a.p = p; a.seed = seed;
    const int epl = dtype == VDM_F32 ? 4 : 8;
    const int ppv = (c1 + c2) / epl;
    a.blocks_per_n = blocks_per_sample(voxels * ppv, ppv, n);
    return a;
}

extern "C" int vdm_gn_silu_fwd(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups, int dtype,
                               const float* stats, const float* gamma, const float* beta, float eps, float dropout_p, uint64_t seed,
                               void* y, uint8_t* keep_mask, int linear, const int32_t* seed_step, void* stream) {
    int e = gn_common_check(c1, c2, n, voxels, groups, dtype, "gn_silu_fwd");
    if (e) return e;
    VDM_REQUIRE(x1 && stats && gamma && beta && y && (c2 == 0 || x2), "gn_silu_fwd: NULL pointer");
    VDM_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "gn_silu_fwd: dropout_p out of range");
    GnArgs a = gn_args(x1, c1, x2, c2, n, voxels, groups, dtype, stats, gamma, beta, eps, dropout_p, seed);
    a.y = y;
    a.mask = keep_mask;
    a.linear = linear != 0;
    a.seed_step = seed_step;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VDM_F32)
        hipLaunchKernelGGL(gn_silu_fwd_kernel<float>, dim3(a.blocks_per_n * n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(gn_silu_fwd_kernel<bf16_t>, dim3(a.blocks_per_n * n), dim3(256), 0, s, a);
    VDM_LAUNCH_CHECK("gn_silu_fwd_kernel");
    return VDM_OK;
}

extern "C" int vdm_gn_dyh(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups, int dtype,
                          const float* stats, const float* gamma, const float* beta, float eps, float dropout_p, uint64_t seed,
                          const void* dy, void* dyh, int linear, const int32_t* seed_step, void* stream) {
    int e = gn_common_check(c1, c2, n, voxels, groups, dtype, "gn_dyh");
    if (e) return e;
    VDM_REQUIRE(x1 && stats && gamma && beta && dy && dyh && (c2 == 0 || x2), "gn_dyh: NULL pointer");
    VDM_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "gn_dyh: dropout_p out of range");
    GnArgs a = gn_args(x1, c1, x2, c2, n, voxels, groups, dtype, stats, gamma, beta, eps, dropout_p, seed);
    a.dy = dy; a.dx1 = dyh;
    a.linear = linear != 0;
    a.seed_step = seed_step;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VDM_F32)
        hipLaunchKernelGGL(gn_dyh_kernel<float>, dim3(a.blocks_per_n * n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(gn_dyh_kernel<bf16_t>, dim3(a.blocks_per_n * n), dim3(256), 0, s, a);
    VDM_LAUNCH_CHECK("gn_dyh_kernel");
    return VDM_OK;
}

extern "C" int vdm_gn_bwd_finalize(const float* partials, int tiles, int n, int c, int groups, int64_t voxels, const float* stats,
                                   const float* gamma, float eps, const float* chsum, float* red, float* chan, float* colsum,
                                   int64_t colsum_stride, void* stream) {
    VDM_REQUIRE(partials && stats && gamma && red && chan, "gn_bwd_finalize: NULL pointer");
    VDM_REQUIRE(tiles > 0 && n > 0 && groups > 0 && c > 0 && c % groups == 0 && voxels > 0, "gn_bwd_finalize: bad sizes");
    VDM_REQUIRE(c / groups <= 256, "gn_bwd_finalize: more than 256 channels per group");
    VDM_REQUIRE(!colsum || chsum, "gn_bwd_finalize: the analytic column sums need the per-channel sums of the GroupNorm input");
    hipLaunchKernelGGL(gn_bwd_finalize_kernel<256>, dim3(n * groups), dim3(256), 0, (hipStream_t)stream, partials, tiles, c, c / groups, voxels,
                       stats, gamma, eps, chsum, red, chan, colsum, (long long)colsum_stride);
    VDM_LAUNCH_CHECK("gn_bwd_finalize_kernel");
    return VDM_OK;
}

extern "C" int vdm_gn_bwd_apply(const void* x1, int c1, const void* x2, int c2, int n, int64_t voxels, int groups, int dtype,
                                const float* stats, const float* gamma, float eps, const void* dyh, const float* red, const float* chan,
                                const void* add1, const void* add2, void* dx1, void* dx2, float* dgamma, float* dbeta, void* stream) {
    int e = gn_common_check(c1, c2, n, voxels, groups, dtype, "gn_bwd_apply");
    if (e) return e;
    VDM_REQUIRE(x1 && stats && gamma && dyh && red && chan && dx1 && dgamma && dbeta && (c2 == 0 || (x2 && dx2)), "gn_bwd_apply: NULL pointer");
    GnArgs a = gn_args(x1, c1, x2, c2, n, voxels, groups, dtype, stats, gamma, gamma, eps, 0.f, 0);
    a.dy = dyh; a.add1 = add1; a.add2 = add2; a.dx1 = dx1; a.dx2 = dx2; a.dgamma = dgamma; a.dbeta = dbeta;
    a.red = const_cast<float*>(red); a.chan = chan;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VDM_F32)
        hipLaunchKernelGGL(gn_bwd_apply_kernel<float>, dim3(a.blocks_per_n * n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(gn_bwd_apply_kernel<bf16_t>, dim3(a.blocks_per_n * n), dim3(256), 0, s, a);
    VDM_LAUNCH_CHECK("gn_bwd_apply_kernel");
    return VDM_OK;
}

extern "C" int vdm_pack_input(const float* a, const float* b, int64_t nvox, int cpad, int dtype, void* out, void* stream) {
    VDM_REQUIRE(a && out && nvox > 0 && cpad >= 2, "pack_input: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VDM_F32)
        hipLaunchKernelGGL(pack_input_kernel<float>, dim3(grid_for(nvox, 256)), dim3(256), 0, s, a, b, nvox, cpad, (float*)out);
    else
        hipLaunchKernelGGL(pack_input_kernel<bf16_t>, dim3(grid_for(nvox, 256)), dim3(256), 0, s, a, b, nvox, cpad, (bf16_t*)out);
    VDM_LAUNCH_CHECK("pack_input_kernel");
    return VDM_OK;
}

// blocks per sample of the two-stage reductions: bpn * n <= VDM_REDUCE_WS_ROWS partial rows as long as n <= VDM_REDUCE_WS_ROWS (the entries
// that write partials require it: the workspace's size is not part of their arguments)
static int bpn_for(int64_t per, int n) {
    int64_t b = (per + 256 * 16 - 1) / (256 * 16);
    int64_t cap = VDM_REDUCE_WS_ROWS / (n > 0 ? n : 1);
    if (cap < 1) cap = 1;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

extern "C" int vdm_diffuse(const float* x, const float* eps, const float* alpha, const float* sigma, int n, int64_t per, float* z_t,
                           void* stream) {
    VDM_REQUIRE(x && eps && alpha && sigma && z_t && n > 0 && per > 0 && per % 4 == 0, "diffuse: bad arguments (per must be a multiple of 4)");
    VDM_REQUIRE((((uintptr_t)x | (uintptr_t)eps | (uintptr_t)z_t) & 15) == 0, "diffuse: x, eps and z_t must be 16-byte aligned");
    const int bpn = bpn_for(per / 4, n);
    hipLaunchKernelGGL(diffuse_kernel, dim3(bpn * n), dim3(256), 0, (hipStream_t)stream, x, eps, alpha, sigma, per, z_t, bpn);
    VDM_LAUNCH_CHECK("diffuse_kernel");
    return VDM_OK;
}

extern "C" int vdm_loss_terms(const float* x, const float* eps, const float* eps_hat, const float* eps0, float s0a0, const float* coef,
                              int n, int64_t per, float* sums, float* d_eps_hat, float* workspace, void* stream) {
    VDM_REQUIRE(x && eps && eps_hat && eps0 && coef && sums && d_eps_hat && workspace && n > 0 && per > 0, "loss_terms: bad arguments");
    VDM_REQUIRE(n <= VDM_REDUCE_WS_ROWS, "loss_terms: at most %d samples per call (got %d): the workspace holds one partial row per block",
                VDM_REDUCE_WS_ROWS, n);
    const int bpn = bpn_for(per, n);
    hipLaunchKernelGGL(loss_terms_kernel, dim3(bpn * n), dim3(256), 0, (hipStream_t)stream, x, eps, eps_hat, eps0, s0a0, coef, per, workspace,
                       d_eps_hat, bpn);
    hipLaunchKernelGGL(fold_partials_kernel, dim3(n * 3), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, bpn, 3, sums, 1);
    VDM_LAUNCH_CHECK("loss_terms_kernel");
    return VDM_OK;
}

// The one launcher of head_kernel: dtype x K for the source's entries (which have refused every k outside KMIN .. KMAX).
template <typename T, int K, typename Src>
static void launch_head_k(const Src& src, int n, int64_t per, float* z, void* packed, hipStream_t s) {
    if constexpr (K >= Src::KMIN && K <= Src::KMAX) {
        const int bpn = bpn_for(per / 4, n);
        hipLaunchKernelGGL((head_kernel<T, K, Src>), dim3(bpn * n), dim3(256), 0, s, src, per, z, (T*)packed, bpn);
    }
}

template <typename T, typename Src>
static void launch_head_t(const Src& src, int k, int n, int64_t per, float* z, void* packed, hipStream_t s) {
    if (k == 0) launch_head_k<T, 0>(src, n, per, z, packed, s);
    else if (k == 1) launch_head_k<T, 1>(src, n, per, z, packed, s);
    else if (k == 2) launch_head_k<T, 2>(src, n, per, z, packed, s);
    else launch_head_k<T, 3>(src, n, per, z, packed, s);
}

template <typename Src>
static int launch_head(const Src& src, int k, int n, int64_t per, int dtype, float* z, void* packed, void* stream) {
    if (dtype == VDM_F32) launch_head_t<float>(src, k, n, per, z, packed, (hipStream_t)stream);
    else launch_head_t<bf16_t>(src, k, n, per, z, packed, (hipStream_t)stream);
    VDM_LAUNCH_CHECK("head_kernel");
    return VDM_OK;
}

extern "C" int vdm_diffuse_pack(const float* x, const float* s_cond, const float* eps, uint64_t seed, uint64_t stream_id,
                                const int32_t* seed_step, const float* alpha, const float* sigma, int n, int64_t per, int dtype, float* z_t,
                                void* packed, void* stream) {
    VDM_REQUIRE(x && alpha && sigma && packed && n > 0 && per > 0 && per % 4 == 0, "diffuse_pack: bad arguments (per must be a multiple of 4)");
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "diffuse_pack: bad dtype %d", dtype);
    VDM_REQUIRE((((uintptr_t)x | (uintptr_t)s_cond | (uintptr_t)eps | (uintptr_t)z_t | (uintptr_t)packed) & 15) == 0,
                "diffuse_pack: x, s_cond, eps, z_t and packed must be 16-byte aligned");
    const DiffuseSrc src = {x, s_cond, eps, seed, stream_id, seed_step, alpha, sigma};
    return launch_head(src, s_cond ? 1 : 0, n, per, dtype, z_t, packed, stream);        // (K = 0: +0 in channel 1)
}

extern "C" int vdm_pack_fields(const float* z, const float* cond, int k, int n, int64_t per, int dtype, void* out, void* stream) {
    VDM_REQUIRE(z && cond && out, "pack_fields: NULL pointer (z, cond and out are required)");
    VDM_REQUIRE(k >= 1 && k <= 3, "pack_fields: %d conditioning fields out of range (1 to 3)", k);
    VDM_REQUIRE(n > 0 && per > 0, "pack_fields: bad sizes n=%d per=%lld", n, (long long)per);
    VDM_REQUIRE(per % 4 == 0, "pack_fields: per=%lld must be a multiple of 4", (long long)per);
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "pack_fields: bad dtype %d", dtype);
    VDM_REQUIRE((((uintptr_t)z | (uintptr_t)cond | (uintptr_t)out) & 15) == 0, "pack_fields: z, cond and out must be 16-byte aligned");
    const PlainSrc src = {z, cond};
    return launch_head(src, k, n, per, dtype, nullptr, out, stream);
}

extern "C" int vdm_diffuse_pack_fields(const float* x, const float* cond, int k, const float* eps, uint64_t seed, uint64_t stream_id,
                                       const int32_t* seed_step, const float* alpha, const float* sigma, int n, int64_t per, int dtype,
                                       float* z_t, void* packed, void* stream) {
    VDM_REQUIRE(x && cond && alpha && sigma && packed, "diffuse_pack_fields: NULL pointer (x, cond, alpha, sigma and packed are required)");
    VDM_REQUIRE(k >= 1 && k <= 3, "diffuse_pack_fields: %d conditioning fields out of range (1 to 3)", k);
    VDM_REQUIRE(n > 0 && per > 0, "diffuse_pack_fields: bad sizes n=%d per=%lld", n, (long long)per);
    VDM_REQUIRE(per % 4 == 0, "diffuse_pack_fields: per=%lld must be a multiple of 4", (long long)per);
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "diffuse_pack_fields: bad dtype %d", dtype);
    VDM_REQUIRE((((uintptr_t)x | (uintptr_t)cond | (uintptr_t)eps | (uintptr_t)z_t | (uintptr_t)packed) & 15) == 0 &&
                    (((uintptr_t)alpha | (uintptr_t)sigma | (uintptr_t)seed_step) & 3) == 0,
                "diffuse_pack_fields: x, cond, eps, z_t and packed must be 16-byte aligned, alpha / sigma / seed_step 4-byte aligned");
    const DiffuseSrc src = {x, cond, eps, seed, stream_id, seed_step, alpha, sigma};
    return launch_head(src, k, n, per, dtype, z_t, packed, stream);
}

extern "C" int vdm_diffuse_pack_fields_keep(const float* x, const float* cond, int k, const float* eps, uint64_t seed, uint64_t stream_id,
                                            const int32_t* seed_step, const float* alpha, const float* sigma, int n, int64_t per,
                                            int dtype, float* z_t, void* packed, const float* keep_s, void* stream) {
    VDM_REQUIRE(x && cond && alpha && sigma && packed,
                "diffuse_pack_fields_keep: NULL pointer (x, cond, alpha, sigma and packed are required)");
    VDM_REQUIRE(k >= 1 && k <= 3, "diffuse_pack_fields_keep: %d conditioning fields out of range (1 to 3)", k);
    VDM_REQUIRE(n > 0 && per > 0, "diffuse_pack_fields_keep: bad sizes n=%d per=%lld", n, (long long)per);
    VDM_REQUIRE(per % 4 == 0, "diffuse_pack_fields_keep: per=%lld must be a multiple of 4", (long long)per);
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "diffuse_pack_fields_keep: bad dtype %d", dtype);
    VDM_REQUIRE((((uintptr_t)x | (uintptr_t)cond | (uintptr_t)eps | (uintptr_t)z_t | (uintptr_t)packed) & 15) == 0 &&
                    (((uintptr_t)alpha | (uintptr_t)sigma | (uintptr_t)seed_step | (uintptr_t)keep_s) & 3) == 0,
                "diffuse_pack_fields_keep: x, cond, eps, z_t and packed must be 16-byte aligned, alpha / sigma / seed_step / keep_s 4-byte "
                "aligned");
    const DiffuseSrc src = {x, cond, eps, seed, stream_id, seed_step, alpha, sigma};
    if (!keep_s) return launch_head(src, k, n, per, dtype, z_t, packed, stream);      // every row kept: vdm_diffuse_pack_fields' kernel
    const DiffuseKeepSrc ksrc = {src, keep_s};
    return launch_head(ksrc, k, n, per, dtype, z_t, packed, stream);
}

extern "C" int vdm_cond_keep(float p, uint64_t seed, const int32_t* seed_step, uint64_t row0, int64_t rows, float* keep, void* stream) {
    VDM_REQUIRE(keep, "cond_keep: keep is NULL");
    VDM_REQUIRE(rows > 0, "cond_keep: rows = %lld (must be positive)", (long long)rows);
    VDM_REQUIRE(p >= 0.f && p <= 1.f, "cond_keep: p = %g outside [0, 1]", (double)p);               // (refuses NaN too)
    VDM_REQUIRE((((uintptr_t)keep | (uintptr_t)seed_step) & 3) == 0, "cond_keep: keep / seed_step must be 4-byte aligned");
    hipLaunchKernelGGL(cond_keep_kernel, dim3(grid_for(rows, 256)), dim3(256), 0, (hipStream_t)stream, p, seed, seed_step, row0, rows, keep);
    VDM_LAUNCH_CHECK("cond_keep_kernel");
    return VDM_OK;
}

extern "C" int vdm_mask_rows(const float* v, const float* keep, int64_t rows, int64_t dim, float* out, void* stream) {
    VDM_REQUIRE(v && keep && out, "mask_rows: NULL pointer (v, keep and out are required)");
    VDM_REQUIRE(rows > 0 && dim > 0, "mask_rows: bad sizes rows=%lld dim=%lld", (long long)rows, (long long)dim);
    VDM_REQUIRE((((uintptr_t)v | (uintptr_t)keep | (uintptr_t)out) & 3) == 0, "mask_rows: v, keep and out must be 4-byte aligned");
    const int vec = (((uintptr_t)v | (uintptr_t)out) & 15) == 0 && dim % 4 == 0;
    int64_t gy = rows < 65535 ? rows : 65535, cap = (2048 + gy - 1) / gy, bx = ((vec ? dim / 4 : dim) + 255) / 256;
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(mask_rows_kernel, dim3((unsigned)bx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, v, keep, rows, dim, vec, out);
    VDM_LAUNCH_CHECK("mask_rows_kernel");
    return VDM_OK;
}

extern "C" int vdm_loss_terms_rng(const float* x, const float* eps, uint64_t seed_eps, uint64_t stream_eps, const float* eps_hat,
                                  const float* eps0, uint64_t seed_eps0, uint64_t stream_eps0, const int32_t* seed_step, float s0a0,
                                  const float* coef, int n, int64_t per, float* sums, float* d_eps_hat, float* workspace, void* stream) {
    VDM_REQUIRE(x && eps_hat && coef && sums && d_eps_hat && workspace && n > 0 && per > 0 && per % 4 == 0,
                "loss_terms_rng: bad arguments (per must be a multiple of 4)");
    VDM_REQUIRE((((uintptr_t)x | (uintptr_t)eps | (uintptr_t)eps_hat | (uintptr_t)eps0 | (uintptr_t)d_eps_hat) & 15) == 0,
                "loss_terms_rng: x, eps, eps_hat, eps0 and d_eps_hat must be 16-byte aligned");
    VDM_REQUIRE(n <= VDM_REDUCE_WS_ROWS, "loss_terms_rng: at most %d samples per call (got %d): the workspace holds one partial row per block",
                VDM_REDUCE_WS_ROWS, n);
    const int bpn = bpn_for(per / 4, n);
    hipLaunchKernelGGL(loss_terms_rng_kernel, dim3(bpn * n), dim3(256), 0, (hipStream_t)stream, x, eps, seed_eps, stream_eps, eps_hat, eps0,
                       seed_eps0, stream_eps0, seed_step, s0a0, coef, per, workspace, d_eps_hat, bpn);
    hipLaunchKernelGGL(fold_partials_kernel, dim3(n * 3), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, bpn, 3, sums, 1);
    VDM_LAUNCH_CHECK("loss_terms_rng_kernel");
    return VDM_OK;
}

extern "C" int vdm_sfm_head(const float* x0, const float* x1, const float* eps, uint64_t seed, uint64_t stream_id, const int32_t* seed_step,
                            const float* t, float sigma, int cond, int n, int64_t per, int dtype, float* x_t, void* packed, void* stream) {
    VDM_REQUIRE(x0 && x1 && t && packed, "sfm_head: NULL pointer (x0, x1, t and packed are required)");
    VDM_REQUIRE(n > 0 && per > 0, "sfm_head: bad sizes n=%d per=%lld", n, (long long)per);
    VDM_REQUIRE(per % 4 == 0, "sfm_head: per=%lld must be a multiple of 4", (long long)per);
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "sfm_head: bad dtype %d", dtype);
    VDM_REQUIRE(sigma >= 0.f, "sfm_head: sigma=%g must be >= 0", (double)sigma);                     // (refuses NaN too)
    VDM_REQUIRE(cond == 0 || cond == 1, "sfm_head: cond=%d must be 0 or 1", cond);
    VDM_REQUIRE((((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)eps | (uintptr_t)x_t | (uintptr_t)packed) & 15) == 0 &&
                    (((uintptr_t)t | (uintptr_t)seed_step) & 3) == 0,
                "sfm_head: x0, x1, eps, x_t and packed must be 16-byte aligned, t / seed_step 4-byte aligned");
    const FlowSrc src = {x0, x1, eps, seed, stream_id, seed_step, t, sigma, cond};
    return launch_head(src, 1, n, per, dtype, x_t, packed, stream);
}

extern "C" int vdm_sfm_loss(const float* v_hat, const float* x0, const float* x1, const float* coef, int n, int64_t per, float* sums,
                            float* d_v, float* workspace, void* stream) {
    VDM_REQUIRE(v_hat && x0 && x1 && coef && sums && d_v && workspace, "sfm_loss: NULL pointer (every argument but stream is required)");
    VDM_REQUIRE(n > 0 && per > 0, "sfm_loss: bad sizes n=%d per=%lld", n, (long long)per);
    VDM_REQUIRE(per % 4 == 0, "sfm_loss: per=%lld must be a multiple of 4", (long long)per);
    VDM_REQUIRE(n <= VDM_REDUCE_WS_ROWS, "sfm_loss: at most %d samples per call (got %d): the workspace holds one partial row per block",
                VDM_REDUCE_WS_ROWS, n);
    VDM_REQUIRE((((uintptr_t)v_hat | (uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)d_v) & 15) == 0 &&
                    (((uintptr_t)coef | (uintptr_t)sums | (uintptr_t)workspace) & 3) == 0,
                "sfm_loss: v_hat, x0, x1 and d_v must be 16-byte aligned, coef / sums / workspace 4-byte aligned");
    const int bpn = bpn_for(per / 4, n);
    hipLaunchKernelGGL(sfm_loss_kernel, dim3(bpn * n), dim3(256), 0, (hipStream_t)stream, v_hat, x0, x1, coef, per, workspace, d_v, bpn);
    hipLaunchKernelGGL(fold_partials_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, bpn, 1, sums, 1);
    VDM_LAUNCH_CHECK("sfm_loss_kernel");
    return VDM_OK;
}

extern "C" int vdm_schedule_grad_sums(const float* dz, const float* x, const float* eps, uint64_t seed_eps, uint64_t stream_eps,
                                      const int32_t* seed_step, int n, int64_t per, float* sums, float* workspace, void* stream) {
    VDM_REQUIRE(dz && x && sums && workspace, "schedule_grad_sums: NULL pointer (dz, x, sums and workspace are required)");
    VDM_REQUIRE(n > 0 && per > 0 && per % 4 == 0, "schedule_grad_sums: bad sizes n=%d per=%lld (per must be a multiple of 4)", n, (long long)per);
    VDM_REQUIRE((((uintptr_t)dz | (uintptr_t)x | (uintptr_t)eps) & 15) == 0, "schedule_grad_sums: dz, x and eps must be 16-byte aligned");
    VDM_REQUIRE(n <= VDM_REDUCE_WS_ROWS, "schedule_grad_sums: at most %d samples per call (got %d): the workspace holds one partial row per block",
                VDM_REDUCE_WS_ROWS, n);
    const int bpn = bpn_for(per / 4, n);
    hipLaunchKernelGGL(schedule_grad_sums_kernel, dim3(bpn * n), dim3(256), 0, (hipStream_t)stream, dz, x, eps, seed_eps, stream_eps, seed_step,
                       per, workspace, bpn);
    hipLaunchKernelGGL(fold_partials_kernel, dim3(n * 2), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, bpn, 2, sums, 0);
    VDM_LAUNCH_CHECK("schedule_grad_sums_kernel");
    return VDM_OK;
}

extern "C" int vdm_ancestral_step(float* z, const float* eps_hat, const float* noise, const float* coef, const int32_t* step_ptr,
                                  uint64_t seed, int64_t n, void* stream) {
    VDM_REQUIRE(z && eps_hat && coef && step_ptr && n > 0, "ancestral_step: bad arguments");
    hipLaunchKernelGGL(ancestral_kernel, dim3(grid_for(n, 256 * 8)), dim3(256), 0, (hipStream_t)stream, z, eps_hat, (const float*)nullptr, 0.f,
                       noise, coef, step_ptr, seed, n);
    VDM_LAUNCH_CHECK("ancestral_kernel");
    return VDM_OK;
}

extern "C" int vdm_ancestral_step_cfg(float* z, const float* eps_cond, const float* eps_uncond, float w_cfg, const float* noise,
                                      const float* coef, const int32_t* step_ptr, uint64_t seed, int64_t n, void* stream) {
    VDM_REQUIRE(z && eps_cond && eps_uncond && coef && step_ptr && n > 0, "ancestral_step_cfg: bad arguments");
    hipLaunchKernelGGL(ancestral_kernel, dim3(grid_for(n, 256 * 8)), dim3(256), 0, (hipStream_t)stream, z, eps_cond, eps_uncond, w_cfg,
                       noise, coef, step_ptr, seed, n);
    VDM_LAUNCH_CHECK("ancestral_kernel(cfg)");
    return VDM_OK;
}

extern "C" int vdm_ancestral_step_rows(float* z, const float* eps_hat, const float* eps_uncond, float w_cfg, const float* coef,
                                       const int32_t* step_ptr, const uint64_t* seeds, int rows, int64_t per_row, void* stream) {
    VDM_REQUIRE(z && eps_hat && coef && step_ptr, "ancestral_step_rows: null z / eps_hat / coef / step_ptr");
    VDM_REQUIRE(seeds, "ancestral_step_rows: seeds is NULL (one device seed per row)");
    VDM_REQUIRE(rows > 0 && rows <= 65535, "ancestral_step_rows: rows = %d (1 .. 65535)", rows);
    VDM_REQUIRE(per_row > 0 && per_row % 4 == 0, "ancestral_step_rows: per_row = %lld (a positive multiple of 4)", (long long)per_row);
    VDM_REQUIRE(((uintptr_t)z | (uintptr_t)eps_hat | (uintptr_t)eps_uncond) % 16 == 0,
                "ancestral_step_rows: z / eps_hat / eps_uncond must be 16-byte aligned");
    // ~2048 workgroups in all, as the one-seed kernel: the rows share the grid, each grid-strides over its own row
    int64_t bx = (per_row / 4 + 255) / 256, cap = (2048 + rows - 1) / rows;
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(ancestral_rows_kernel, dim3((unsigned)bx, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, z, eps_hat, eps_uncond,
                       w_cfg, coef, step_ptr, seeds, per_row);
    VDM_LAUNCH_CHECK("ancestral_rows_kernel");
    return VDM_OK;
}

extern "C" int vdm_multistep_step(float* z, const float* eps_hat, const float* eps_uncond, float w_cfg, float* prev, const float* coef,
                                  const int32_t* step_ptr, int64_t n, void* stream) {
    VDM_REQUIRE(z && eps_hat && prev && coef && step_ptr, "multistep_step: null z / eps_hat / prev / coef / step_ptr");
    VDM_REQUIRE(n > 0, "multistep_step: n = %lld (must be positive)", (long long)n);
    const bool aligned = (((uintptr_t)z | (uintptr_t)eps_hat | (uintptr_t)eps_uncond | (uintptr_t)prev) & 15) == 0;
    hipLaunchKernelGGL(multistep_kernel, dim3(grid_for(n, 256 * 8)), dim3(256), 0, (hipStream_t)stream, z, eps_hat, eps_uncond, w_cfg, prev,
                       coef, step_ptr, aligned ? n >> 2 : (int64_t)0, n);
    VDM_LAUNCH_CHECK("multistep_kernel");
    return VDM_OK;
}

extern "C" int vdm_channel_sums(const void* x, int64_t rows, int c, int dtype, float* out, void* stream) {
    VDM_REQUIRE(x && out && rows > 0 && c > 0, "channel_sums: bad arguments");
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "channel_sums: dtype");
    const int epl = dtype == VDM_F32 ? 4 : 8;
    VDM_REQUIRE(c % epl == 0, "channel_sums: channels must be a multiple of %d", epl);
    if (dtype == VDM_F32)
        hipLaunchKernelGGL(channel_sums_kernel<float>, dim3(c / epl), dim3(256), 0, (hipStream_t)stream, (const float*)x, rows, c, out);
    else
        hipLaunchKernelGGL(channel_sums_kernel<bf16_t>, dim3(c / epl), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, rows, c, out);
    VDM_LAUNCH_CHECK("channel_sums_kernel");
    return VDM_OK;
}

extern "C" int vdm_channel_dot_sums(const void* a, const void* b1, int c1, const void* b2, int c2, int n, int64_t rows_per_sample, int dtype,
                                    float* out, void* stream) {
    VDM_REQUIRE(a && b1 && out && n > 0 && rows_per_sample > 0 && c1 > 0 && c2 >= 0 && (c2 == 0 || b2), "channel_dot_sums: bad arguments");
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "channel_dot_sums: dtype");
    const int epl = dtype == VDM_F32 ? 4 : 8;
    VDM_REQUIRE(c1 % epl == 0 && c2 % epl == 0, "channel_dot_sums: channel counts must be multiples of %d", epl);
    if (dtype == VDM_F32)
        hipLaunchKernelGGL(channel_dot_sums_kernel<float>, dim3((c1 + c2) / epl, n), dim3(256), 0, (hipStream_t)stream, (const float*)a,
                           (const float*)b1, c1, (const float*)b2, c2, rows_per_sample, out);
    else
        hipLaunchKernelGGL(channel_dot_sums_kernel<bf16_t>, dim3((c1 + c2) / epl, n), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)a,
                           (const bf16_t*)b1, c1, (const bf16_t*)b2, c2, rows_per_sample, out);
    VDM_LAUNCH_CHECK("channel_dot_sums_kernel");
    return VDM_OK;
}

extern "C" int vdm_randn(float* out, int64_t n, uint64_t seed, uint64_t stream_id, const int32_t* seed_step, void* stream) {
    VDM_REQUIRE(out && n > 0, "randn: bad arguments");
    hipLaunchKernelGGL(randn_kernel, dim3(grid_for(n, 256 * 8)), dim3(256), 0, (hipStream_t)stream, out, n, seed, stream_id, seed_step);
    VDM_LAUNCH_CHECK("randn_kernel");
    return VDM_OK;
}

extern "C" int vdm_step_inc(int32_t* step_ptr, void* stream) {
    VDM_REQUIRE(step_ptr, "step_inc: NULL pointer");
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_ptr);
    VDM_LAUNCH_CHECK("step_inc_kernel");
    return VDM_OK;
}

extern "C" int vdm_sumsq(const float* x, int64_t n, float* out, float* workspace, void* stream) {
    VDM_REQUIRE(x && out && workspace && n > 0, "sumsq: bad arguments");
    VDM_REQUIRE(((uintptr_t)x & 15) == 0, "sumsq: x must be 16-byte aligned");
    const unsigned g = grid_for(n, 256 * 16);
    hipLaunchKernelGGL(sumsq_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, x, n, workspace);
    hipLaunchKernelGGL(fold_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, (int)g, 1, out, 1);
    VDM_LAUNCH_CHECK("sumsq_kernel");
    return VDM_OK;
}

extern "C" int vdm_train_scalars(const float* u0, const float* times, int batch, int rank, int world, float gamma_min, float gamma_max,
                                 float bpd_over_batch, float* out, uint64_t seed, const int32_t* seed_step, void* stream) {
    VDM_REQUIRE(out && batch > 0 && world > 0 && rank >= 0 && rank < world, "train_scalars: bad arguments");
    VDM_REQUIRE(gamma_max > gamma_min, "train_scalars: gamma_max must exceed gamma_min");
    hipLaunchKernelGGL(train_scalars_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream, u0, times, batch, rank, world, gamma_min,
                       gamma_max, bpd_over_batch, out, seed, seed_step);
    VDM_LAUNCH_CHECK("train_scalars_kernel");
    return VDM_OK;
}

extern "C" int vdm_elbo_assemble(const float* sums, const float* coef, int batch, float c_lat0, float c_lat1, float c_rec0, float c_rec1,
                                 float* out, void* stream) {
    VDM_REQUIRE(sums && coef && out && batch > 0, "elbo_assemble: bad arguments");
    hipLaunchKernelGGL(elbo_assemble_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, coef, batch, c_lat0, c_lat1, c_rec0, c_rec1, out);
    VDM_LAUNCH_CHECK("elbo_assemble_kernel");
    return VDM_OK;
}

extern "C" int vdm_clip_scale(float* x, int64_t n, const float* sumsq, float max_norm, void* stream) {
    VDM_REQUIRE(x && sumsq && n > 0 && max_norm > 0.f, "clip_scale: bad arguments");
    VDM_REQUIRE(((uintptr_t)x & 15) == 0, "clip_scale: x must be 16-byte aligned");
    hipLaunchKernelGGL(clip_scale_kernel, dim3(grid_for(n, 256 * 16)), dim3(256), 0, (hipStream_t)stream, x, n, sumsq, max_norm);
    VDM_LAUNCH_CHECK("clip_scale_kernel");
    return VDM_OK;
}
