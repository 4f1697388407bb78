// ddnm.hip - the DDNM range/null-space sampler's update as HBM-bound fp32 kernels (K11 of DESIGN.md) [REF src/utils.py:277-304]:
//   x_0t = (z - sigma_t eps_hat) / alpha_t ;  x_r = AT y + x_0t - AT A x_0t ;  z <- w_z z + w_x x_r + scale noise
// for a generic operator (x0 kernel, the caller's AT(A(.)), update kernel), fused for A = AT = mask and for A = block mean /
// AT = nearest up-sampling, plus the travel-back z <- a z + b noise and the cursor advance.
// Every kernel reads its scalars from DEVICE tables at a device-side cursor (one captured graph serves all evaluations):
//   e = *cursor (evaluation index, monotonic), (k, draw) = sched[e], coef[k][8] = {1/alpha_t, sigma_t, w_z, w_x, scale, t_norm, 0, 0};
// the noise of row r is supplied, or the Philox normal of (seeds[r], draw + 1, float4 group within the row) - the field
// vdm_randn(seeds[r], stream_id = draw + 1) writes for one row (batch_stream: one stream over the whole batch, seeds[0]).
// All element arithmetic goes through ddnm_x0 / ddnm_xr / ddnm_z with the rounding spelled out, so the fused kernels and the generic
// pair give the same bits wherever the operator's own arithmetic is the same.
#include "common.h"

namespace vdm {

struct DdnmScalars {
    float inv_a, sigma_t, w_z, w_x, scale;
    uint64_t sid;            // Philox stream id of this evaluation's draw
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ DdnmScalars ddnm_scalars(const vdm_ddnm_tables& t) {
    const int e = clampi(*t.cursor, t.n_sched - 1);           // (clamped: a cursor run past the schedule never reads outside the tables)
    const int k = clampi(t.sched[2 * e], t.n_coef - 1);
    const float* c = t.coef + (size_t)k * 8;
    DdnmScalars s;
    s.inv_a = c[0]; s.sigma_t = c[1]; s.w_z = c[2]; s.w_x = c[3]; s.scale = c[4];
    s.sid = (uint64_t)(int64_t)t.sched[2 * e + 1] + 1u;
    return s;
}

__device__ __forceinline__ float ddnm_x0(float z, float eh, float eu, bool cfg, float w, float sigma_t, float inv_a) {
    const float e = cfg ? uncontracted_mul(1.f + w, eh) - uncontracted_mul(w, eu) : eh;     // the blend of K9
    return uncontracted_mul(fmaf(-sigma_t, e, z), inv_a);
}
__device__ __forceinline__ float ddnm_xr(float aty, float x0, float atax0) { return (aty + x0) - atax0; }
__device__ __forceinline__ float ddnm_z(float z, float xr, float nz, float w_z, float w_x, float scale) {
    return (uncontracted_mul(w_z, z) + uncontracted_mul(w_x, xr)) + uncontracted_mul(scale, nz);
}

// seed and float4-group offset of row r
struct RowNoise {
    const float4* field;     // supplied noise of this row, or NULL
    uint64_t seed, off;
    __device__ __forceinline__ float4 at(uint64_t sid, int64_t i) const { return field ? field[i] : randn4(seed, sid, off + (uint64_t)i); }
};
__device__ __forceinline__ RowNoise row_noise(const float* noise, const vdm_ddnm_tables& t, int r, int64_t per) {
    RowNoise n;
    n.field = noise ? reinterpret_cast<const float4*>(noise + (size_t)r * per) : nullptr;
    n.seed = noise ? 0 : (t.batch_stream ? t.seeds[0] : t.seeds[r]);
    n.off = t.batch_stream ? (uint64_t)r * (uint64_t)(per >> 2) : 0;
    return n;
}

// ---- generic operator: x_0t, then (after the caller's AT(A(x_0t))) the update --------------------------------------------------------
__global__ void __launch_bounds__(256) ddnm_x0_kernel(const float* __restrict__ z, const float* __restrict__ eh, const float* __restrict__ eu,
                                                     float w, vdm_ddnm_tables t, float* __restrict__ x0, int64_t n4) {
    const DdnmScalars s = ddnm_scalars(t);
    const float4* z4 = reinterpret_cast<const float4*>(z);
    const float4* h4 = reinterpret_cast<const float4*>(eh);
    const float4* u4 = eu ? reinterpret_cast<const float4*>(eu) : nullptr;
    float4* o4 = reinterpret_cast<float4*>(x0);
    const bool cfg = u4 != nullptr;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 zv = z4[i], hv = h4[i], uv = cfg ? u4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 o;
        o.x = ddnm_x0(zv.x, hv.x, uv.x, cfg, w, s.sigma_t, s.inv_a);
        o.y = ddnm_x0(zv.y, hv.y, uv.y, cfg, w, s.sigma_t, s.inv_a);
        o.z = ddnm_x0(zv.z, hv.z, uv.z, cfg, w, s.sigma_t, s.inv_a);
        o.w = ddnm_x0(zv.w, hv.w, uv.w, cfg, w, s.sigma_t, s.inv_a);
        o4[i] = o;
    }
}

__global__ void __launch_bounds__(256) ddnm_update_kernel(float* __restrict__ z, const float* __restrict__ x0, const float* __restrict__ ata,
                                                         const float* __restrict__ aty, int aty_rows, const float* __restrict__ noise,
                                                         vdm_ddnm_tables t, float* __restrict__ xr, int64_t per) {
    const DdnmScalars s = ddnm_scalars(t);
    const int r = blockIdx.y;
    const size_t base = (size_t)r * per;
    const RowNoise nz = row_noise(noise, t, r, per);
    float4* z4 = reinterpret_cast<float4*>(z + base);
    const float4* x4 = reinterpret_cast<const float4*>(x0 + base);
    const float4* a4 = reinterpret_cast<const float4*>(ata + base);
    const float4* y4 = reinterpret_cast<const float4*>(aty + (aty_rows == 1 ? 0 : base));
    float4* r4 = xr ? reinterpret_cast<float4*>(xr + base) : nullptr;
    const int64_t n4 = per >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 nv = nz.at(s.sid, i), xv = x4[i], av = a4[i], yv = y4[i];
        float4 zv = z4[i], o;
        o.x = ddnm_xr(yv.x, xv.x, av.x); o.y = ddnm_xr(yv.y, xv.y, av.y); o.z = ddnm_xr(yv.z, xv.z, av.z); o.w = ddnm_xr(yv.w, xv.w, av.w);
        zv.x = ddnm_z(zv.x, o.x, nv.x, s.w_z, s.w_x, s.scale);
        zv.y = ddnm_z(zv.y, o.y, nv.y, s.w_z, s.w_x, s.scale);
        zv.z = ddnm_z(zv.z, o.z, nv.z, s.w_z, s.w_x, s.scale);
        zv.w = ddnm_z(zv.w, o.w, nv.w, s.w_z, s.w_x, s.scale);
        z4[i] = zv;
        if (r4) r4[i] = o;
    }
}

// ---- A = AT = mask: x_0t, x_r = m y + x_0t - m (m x_0t), the z update and the noise in one pass ----------------------------------------
__device__ __forceinline__ float mask_xr(float m, float y, float x0) {
    return ddnm_xr(uncontracted_mul(m, y), x0, uncontracted_mul(m, uncontracted_mul(m, x0)));
}

__global__ void __launch_bounds__(256) ddnm_mask_kernel(float* __restrict__ z, const float* __restrict__ eh, const float* __restrict__ eu, float w,
                                                       const float* __restrict__ mask, int mask_rows, const float* __restrict__ y, int y_rows,
                                                       const float* __restrict__ noise, vdm_ddnm_tables t, float* __restrict__ xr, int64_t per) {
    const DdnmScalars s = ddnm_scalars(t);
    const int r = blockIdx.y;
    const size_t base = (size_t)r * per;
    const RowNoise nz = row_noise(noise, t, r, per);
    float4* z4 = reinterpret_cast<float4*>(z + base);
    const float4* h4 = reinterpret_cast<const float4*>(eh + base);
    const float4* u4 = eu ? reinterpret_cast<const float4*>(eu + base) : nullptr;
    const float4* m4 = reinterpret_cast<const float4*>(mask + (mask_rows == 1 ? 0 : base));
    const float4* y4 = reinterpret_cast<const float4*>(y + (y_rows == 1 ? 0 : base));
    float4* r4 = xr ? reinterpret_cast<float4*>(xr + base) : nullptr;
    const bool cfg = u4 != nullptr;
    const int64_t n4 = per >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 nv = nz.at(s.sid, i), hv = h4[i], uv = cfg ? u4[i] : make_float4(0.f, 0.f, 0.f, 0.f), mv = m4[i], yv = y4[i];
        float4 zv = z4[i], o;
        o.x = mask_xr(mv.x, yv.x, ddnm_x0(zv.x, hv.x, uv.x, cfg, w, s.sigma_t, s.inv_a));
        o.y = mask_xr(mv.y, yv.y, ddnm_x0(zv.y, hv.y, uv.y, cfg, w, s.sigma_t, s.inv_a));
        o.z = mask_xr(mv.z, yv.z, ddnm_x0(zv.z, hv.z, uv.z, cfg, w, s.sigma_t, s.inv_a));
        o.w = mask_xr(mv.w, yv.w, ddnm_x0(zv.w, hv.w, uv.w, cfg, w, s.sigma_t, s.inv_a));
        zv.x = ddnm_z(zv.x, o.x, nv.x, s.w_z, s.w_x, s.scale);
        zv.y = ddnm_z(zv.y, o.y, nv.y, s.w_z, s.w_x, s.scale);
        zv.z = ddnm_z(zv.z, o.z, nv.z, s.w_z, s.w_x, s.scale);
        zv.w = ddnm_z(zv.w, o.w, nv.w, s.w_z, s.w_x, s.scale);
        z4[i] = zv;
        if (r4) r4[i] = o;
    }
}

// ---- A = mean over fz x fy x fx blocks, AT = nearest up-sampling ----------------------------------------------------------------------
// A thread owns one float4 column of a block: the 4 consecutive x voxels at x4, over the block's fz * fy rows.  Pass 1 forms x_0t row by row
// and adds the rows in registers; the x direction folds inside the float4 (fx = 2, 4) and with the neighbour lane (fx = 8: one
// __shfl_xor - lanes 2j, 2j + 1 hold the two halves of a block, both always active since W / 4 is even).  Pass 2 re-reads the block's
// rows (just read by the same thread: L1/L2 hits, not HBM), recomputes x_0t - same instructions, same bits - and does
// x_r = (y_block + x_0t) - mean, the z update and the noise.  HBM traffic: z, eps_hat (and y / fz fy fx) read, z and x_r written.
__global__ void __launch_bounds__(256) ddnm_blockmean_kernel(float* __restrict__ z, const float* __restrict__ eh, const float* __restrict__ eu,
                                                            float w, const float* __restrict__ y, int y_rows, int D, int H, int W, int fz, int fy,
                                                            int fx, const float* __restrict__ noise, vdm_ddnm_tables t, float* __restrict__ xr) {
    const DdnmScalars s = ddnm_scalars(t);
    const int r = blockIdx.y;
    const int W4 = W >> 2, Hb = H / fy, Db = D / fz, Wb = W / fx;
    const int64_t per = (int64_t)D * H * W;
    const size_t base = (size_t)r * per;
    const RowNoise nz = row_noise(noise, t, r, per);
    float4* z4 = reinterpret_cast<float4*>(z + base);
    const float4* h4 = reinterpret_cast<const float4*>(eh + base);
    const float4* u4 = eu ? reinterpret_cast<const float4*>(eu + base) : nullptr;
    float4* r4 = xr ? reinterpret_cast<float4*>(xr + base) : nullptr;
    const float* yb = y + (y_rows == 1 ? (size_t)0 : (size_t)r * Db * Hb * Wb);
    const bool cfg = u4 != nullptr;
    const float inv_cnt = 1.f / (float)(fz * fy * fx);            // a power of two: exact
    const int64_t ncol = (int64_t)Db * Hb * W4;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < ncol; c += (int64_t)gridDim.x * 256) {
        const int x4 = (int)(c % W4);
        const int64_t br = c / W4;
        const int by = (int)(br % Hb), bz = (int)(br / Hb);
        const int64_t first = ((int64_t)bz * fz * H + (int64_t)by * fy) * W4 + x4;      // float4 index of the block's first row
        float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int iz = 0; iz < fz; ++iz) {                         // (per-plane partial sums: at most 8 + 8 + 3 additions deep)
            float4 ps = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int iy = 0; iy < fy; ++iy) {
                const int64_t i = first + ((int64_t)iz * H + iy) * W4;
                const float4 zv = z4[i], hv = h4[i], uv = cfg ? u4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
                ps.x += ddnm_x0(zv.x, hv.x, uv.x, cfg, w, s.sigma_t, s.inv_a);
                ps.y += ddnm_x0(zv.y, hv.y, uv.y, cfg, w, s.sigma_t, s.inv_a);
                ps.z += ddnm_x0(zv.z, hv.z, uv.z, cfg, w, s.sigma_t, s.inv_a);
                ps.w += ddnm_x0(zv.w, hv.w, uv.w, cfg, w, s.sigma_t, s.inv_a);
            }
            sum.x += ps.x; sum.y += ps.y; sum.z += ps.z; sum.w += ps.w;
        }
        if (fx == 2) {
            const float a = sum.x + sum.y, b = sum.z + sum.w;
            sum = make_float4(a, a, b, b);
        } else if (fx >= 4) {
            float a = (sum.x + sum.y) + (sum.z + sum.w);
            if (fx == 8) a += __shfl_xor(a, 1, 64);
            sum = make_float4(a, a, a, a);
        }
        const float4 mean = make_float4(sum.x * inv_cnt, sum.y * inv_cnt, sum.z * inv_cnt, sum.w * inv_cnt);
        const float* yrow = yb + ((size_t)bz * Hb + by) * Wb;
        const int xe = x4 * 4;
        const float4 yv = make_float4(yrow[xe / fx], yrow[(xe + 1) / fx], yrow[(xe + 2) / fx], yrow[(xe + 3) / fx]);
        for (int iz = 0; iz < fz; ++iz)
            for (int iy = 0; iy < fy; ++iy) {
                const int64_t i = first + ((int64_t)iz * H + iy) * W4;
                const float4 nv = nz.at(s.sid, i), hv = h4[i], uv = cfg ? u4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
                float4 zv = z4[i], o;
                o.x = ddnm_xr(yv.x, ddnm_x0(zv.x, hv.x, uv.x, cfg, w, s.sigma_t, s.inv_a), mean.x);
                o.y = ddnm_xr(yv.y, ddnm_x0(zv.y, hv.y, uv.y, cfg, w, s.sigma_t, s.inv_a), mean.y);
                o.z = ddnm_xr(yv.z, ddnm_x0(zv.z, hv.z, uv.z, cfg, w, s.sigma_t, s.inv_a), mean.z);
                o.w = ddnm_xr(yv.w, ddnm_x0(zv.w, hv.w, uv.w, cfg, w, s.sigma_t, s.inv_a), mean.w);
                zv.x = ddnm_z(zv.x, o.x, nv.x, s.w_z, s.w_x, s.scale);
                zv.y = ddnm_z(zv.y, o.y, nv.y, s.w_z, s.w_x, s.scale);
                zv.z = ddnm_z(zv.z, o.z, nv.z, s.w_z, s.w_x, s.scale);
                zv.w = ddnm_z(zv.w, o.w, nv.w, s.w_z, s.w_x, s.scale);
                z4[i] = zv;
                if (r4) r4[i] = o;
            }
    }
}

// ---- travel back L steps: z <- a z + b noise, {a, b} = travel[outer][2]; the draw number comes from the host loop ----------------------
__global__ void __launch_bounds__(256) ddnm_travel_kernel(float* __restrict__ z, const float* __restrict__ noise, vdm_ddnm_tables t,
                                                         const float* __restrict__ travel, int outer, uint64_t sid, int64_t per) {
    const float a = travel[2 * outer], b = travel[2 * outer + 1];
    const int r = blockIdx.y;
    const RowNoise nz = row_noise(noise, t, r, per);
    float4* z4 = reinterpret_cast<float4*>(z + (size_t)r * per);
    const int64_t n4 = per >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 nv = nz.at(sid, i);
        float4 zv = z4[i];
        zv.x = uncontracted_mul(a, zv.x) + uncontracted_mul(b, nv.x);
        zv.y = uncontracted_mul(a, zv.y) + uncontracted_mul(b, nv.y);
        zv.z = uncontracted_mul(a, zv.z) + uncontracted_mul(b, nv.z);
        zv.w = uncontracted_mul(a, zv.w) + uncontracted_mul(b, nv.w);
        z4[i] = zv;
    }
}

// *cursor += 1 and *k_ptr = k of the next evaluation (where vdm_cond_table_step reads its row index)
__global__ void ddnm_advance_kernel(int32_t* cursor, const int32_t* __restrict__ sched, int n_sched, int32_t* k_ptr) {
    const int e = *cursor + 1;
    *cursor = e;
    *k_ptr = sched[2 * clampi(e, n_sched - 1)];
}

// rows share ~2048 workgroups, each grid-strides over its own row (as vdm_ancestral_step_rows)
static inline unsigned row_blocks(int64_t items, int rows) {
    int64_t bx = (items + 255) / 256, cap = (2048 + rows - 1) / rows;
    if (bx > cap) bx = cap;
    return (unsigned)(bx < 1 ? 1 : bx);
}

static int check_tables(const vdm_ddnm_tables* t, const float* noise, const char* who) {
    VDM_REQUIRE(t && t->coef && t->sched && t->cursor, "%s: tables / coef / sched / cursor is NULL", who);
    VDM_REQUIRE(t->n_coef > 0 && t->n_sched > 0, "%s: n_coef = %d, n_sched = %d (both positive)", who, t->n_coef, t->n_sched);
    VDM_REQUIRE(noise || t->seeds, "%s: neither a noise field nor a seed table", who);
    return VDM_OK;
}

static int check_rows(int rows, int64_t per_row, const char* who) {
    VDM_REQUIRE(rows > 0 && rows <= 65535, "%s: rows = %d (1 .. 65535)", who, rows);
    VDM_REQUIRE(per_row > 0 && per_row % 4 == 0, "%s: per_row = %lld (a positive multiple of 4)", who, (long long)per_row);
    return VDM_OK;
}

#define DDNM_ALIGNED(...) ((vdm::or_ptrs(__VA_ARGS__) & 15) == 0)
template <typename... P> static inline uintptr_t or_ptrs(P... p) { return (... | (uintptr_t)p); }

}  // namespace vdm

using namespace vdm;

extern "C" int vdm_ddnm_x0(const float* z, const float* eps_hat, const float* eps_uncond, float w_cfg, const vdm_ddnm_tables* tables,
                           float* x0, int64_t n, void* stream) {
    VDM_REQUIRE(z && eps_hat && x0, "ddnm_x0: null z / eps_hat / x0");
    VDM_REQUIRE(tables && tables->coef && tables->sched && tables->cursor && tables->n_coef > 0 && tables->n_sched > 0, "ddnm_x0: bad tables");
    VDM_REQUIRE(n > 0 && n % 4 == 0, "ddnm_x0: n = %lld (a positive multiple of 4)", (long long)n);
    VDM_REQUIRE(DDNM_ALIGNED(z, eps_hat, eps_uncond, x0), "ddnm_x0: the fields must be 16-byte aligned");
    hipLaunchKernelGGL(ddnm_x0_kernel, dim3(row_blocks(n / 4, 1)), dim3(256), 0, (hipStream_t)stream, z, eps_hat, eps_uncond, w_cfg, *tables, x0,
                       n / 4);
    VDM_LAUNCH_CHECK("ddnm_x0_kernel");
    return VDM_OK;
}

extern "C" int vdm_ddnm_update(float* z, const float* x0, const float* atax0, const float* aty, int aty_rows, const float* noise,
                               const vdm_ddnm_tables* tables, float* x_r, int rows, int64_t per_row, void* stream) {
    VDM_REQUIRE(z && x0 && atax0 && aty, "ddnm_update: null z / x0 / atax0 / aty");
    if (int e = check_tables(tables, noise, "ddnm_update")) return e;
    if (int e = check_rows(rows, per_row, "ddnm_update")) return e;
    VDM_REQUIRE(aty_rows == 1 || aty_rows == rows, "ddnm_update: aty_rows = %d (1 or rows = %d)", aty_rows, rows);
    VDM_REQUIRE(DDNM_ALIGNED(z, x0, atax0, aty, noise, x_r), "ddnm_update: the fields must be 16-byte aligned");
    hipLaunchKernelGGL(ddnm_update_kernel, dim3(row_blocks(per_row / 4, rows), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, z, x0, atax0,
                       aty, aty_rows, noise, *tables, x_r, per_row);
    VDM_LAUNCH_CHECK("ddnm_update_kernel");
    return VDM_OK;
}

extern "C" int vdm_ddnm_mask_step(float* z, const float* eps_hat, const float* eps_uncond, float w_cfg, const float* mask, int mask_rows,
                                  const float* y, int y_rows, const float* noise, const vdm_ddnm_tables* tables, float* x_r, int rows,
                                  int64_t per_row, void* stream) {
    VDM_REQUIRE(z && eps_hat && mask && y, "ddnm_mask_step: null z / eps_hat / mask / y");
    if (int e = check_tables(tables, noise, "ddnm_mask_step")) return e;
    if (int e = check_rows(rows, per_row, "ddnm_mask_step")) return e;
    VDM_REQUIRE((mask_rows == 1 || mask_rows == rows) && (y_rows == 1 || y_rows == rows),
                "ddnm_mask_step: mask_rows = %d, y_rows = %d (1 or rows = %d)", mask_rows, y_rows, rows);
    VDM_REQUIRE(DDNM_ALIGNED(z, eps_hat, eps_uncond, mask, y, noise, x_r), "ddnm_mask_step: the fields must be 16-byte aligned");
    hipLaunchKernelGGL(ddnm_mask_kernel, dim3(row_blocks(per_row / 4, rows), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, z, eps_hat,
                       eps_uncond, w_cfg, mask, mask_rows, y, y_rows, noise, *tables, x_r, per_row);
    VDM_LAUNCH_CHECK("ddnm_mask_kernel");
    return VDM_OK;
}

extern "C" int vdm_ddnm_blockmean_step(float* z, const float* eps_hat, const float* eps_uncond, float w_cfg, const float* y, int y_rows, int d,
                                       int h, int w, int fz, int fy, int fx, const float* noise, const vdm_ddnm_tables* tables, float* x_r,
                                       int rows, void* stream) {
    VDM_REQUIRE(z && eps_hat && y, "ddnm_blockmean_step: null z / eps_hat / y");
    if (int e = check_tables(tables, noise, "ddnm_blockmean_step")) return e;
    VDM_REQUIRE(d > 0 && h > 0 && w > 0 && d <= 65536 && h <= 65536 && w <= 65536, "ddnm_blockmean_step: cube %d x %d x %d", d, h, w);
    for (int f : {fz, fy, fx}) VDM_REQUIRE(f == 1 || f == 2 || f == 4 || f == 8, "ddnm_blockmean_step: factor %d (1, 2, 4 or 8)", f);
    VDM_REQUIRE(d % fz == 0 && h % fy == 0 && w % fx == 0 && w % 4 == 0,
                "ddnm_blockmean_step: factors (%d, %d, %d) must divide the cube %d x %d x %d, and x be a multiple of 4", fz, fy, fx, d, h, w);
    if (int e = check_rows(rows, (int64_t)d * h * w, "ddnm_blockmean_step")) return e;
    VDM_REQUIRE(y_rows == 1 || y_rows == rows, "ddnm_blockmean_step: y_rows = %d (1 or rows = %d)", y_rows, rows);
    VDM_REQUIRE(DDNM_ALIGNED(z, eps_hat, eps_uncond, noise, x_r), "ddnm_blockmean_step: the fields must be 16-byte aligned");
    const int64_t ncol = (int64_t)(d / fz) * (h / fy) * (w / 4);
    hipLaunchKernelGGL(ddnm_blockmean_kernel, dim3(row_blocks(ncol, rows), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, z, eps_hat,
                       eps_uncond, w_cfg, y, y_rows, d, h, w, fz, fy, fx, noise, *tables, x_r);
    VDM_LAUNCH_CHECK("ddnm_blockmean_kernel");
    return VDM_OK;
}

extern "C" int vdm_ddnm_travel(float* z, const float* noise, const vdm_ddnm_tables* tables, const float* travel, int outer, int64_t draw,
                               int rows, int64_t per_row, void* stream) {
    VDM_REQUIRE(z && travel && outer >= 0 && draw >= 0, "ddnm_travel: null z / travel, or a negative outer / draw");
    VDM_REQUIRE(tables && (noise || tables->seeds), "ddnm_travel: neither a noise field nor a seed table");
    if (int e = check_rows(rows, per_row, "ddnm_travel")) return e;
    VDM_REQUIRE(DDNM_ALIGNED(z, noise), "ddnm_travel: the fields must be 16-byte aligned");
    hipLaunchKernelGGL(ddnm_travel_kernel, dim3(row_blocks(per_row / 4, rows), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, z, noise, *tables,
                       travel, outer, (uint64_t)draw + 1u, per_row);
    VDM_LAUNCH_CHECK("ddnm_travel_kernel");
    return VDM_OK;
}

extern "C" int vdm_ddnm_advance(int32_t* cursor, const int32_t* sched, int n_sched, int32_t* k_ptr, void* stream) {
    VDM_REQUIRE(cursor && sched && k_ptr && n_sched > 0, "ddnm_advance: null cursor / sched / k_ptr, or n_sched <= 0");
    hipLaunchKernelGGL(ddnm_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, cursor, sched, n_sched, k_ptr);
    VDM_LAUNCH_CHECK("ddnm_advance_kernel");
    return VDM_OK;
}
