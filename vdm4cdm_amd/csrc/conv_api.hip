// conv_api.hip - weight packing kernels and the C-ABI entry points of the convolutions (see conv_common.h).
#include <algorithm>

#include "conv_common.h"

using namespace vdm;

// ---- all weight packings of a network in ONE launch ---------------------------------------------------------------------
// The packed copies of every conv (forward and dgrad form) are rebuilt after each optimiser step: ~120 launches of a few
// microseconds each when done conv by conv.  vdm_conv_pack_plan() fills one work item per (conv, form) on the host; the caller
// concatenates them, cuts the concatenated element range into chunks of VDM_PACK_CHUNK elements that do not straddle items, uploads
// both tables once and calls vdm_conv_pack_many() per step.
__device__ ClsMasks g_cls_masks[3];

// The ONE definition of the three packed layouts (master fp32 [taps][cout][cin] -> MFMA A-fragment order): the value of packed
// element (row r = everything above the [lane][EPL] fragment, lane (m = lane&15, q = lane>>4), j).  In all of them
//     out channel o = chunk*NC*16 + NC*4*(m>>2) + 4*ct + (m&3);   fwd reads W[tap][o][k], dgrad W[flip(tap)][k][o] (o indexes cin)
//   generic     packed[chunk][kb][tap][ct][lane][EPL]:     reduction channel k = kb*KB + q*EPL + j
//   class       packed[chunk][kb][slot 0..63][ct][lane][EPL] = sum over the master taps in mask[slot], ascending (dgrad: W[t][k][o])
//   tap-packed  packed[chunk][tap group g 0..6][ct][lane][ci 0..7] = W[tap 4g+q][o][ci]    (conv_kpack_kernel)
template <typename T>
__device__ __forceinline__ float pack_value(const vdm_pack_item& it, const float* __restrict__ w, size_t r, int lane, int j) {
    constexpr int EPL = DT<T>::EPL, KB = DT<T>::KB;
    const int dgrad = it.dgrad, cout_m = it.cout, cin_m = it.cin, nc = it.nc;
    const int O = dgrad ? cin_m : cout_m, K = dgrad ? cout_m : cin_m;
    const int ct = r % nc; r /= nc;
    const int m = lane & 15, q = lane >> 4;
    if (it.variant == VDM_CONV_VARIANT_KPACK) {
        const int g = r % 7; r /= 7;
        const int chunk = (int)r;
        const int o = chunk * nc * 16 + nc * 4 * (m >> 2) + 4 * ct + (m & 3);
        const int tap = 4 * g + q;
        if (!(o < O && j < K && tap < 27)) return 0.f;
        return dgrad ? w[((size_t)(26 - tap) * cout_m + j) * cin_m + o] : w[((size_t)tap * cout_m + o) * cin_m + j];
    }
    if (it.variant == VDM_CONV_VARIANT_CLASS) {
        const int slot = r % 64; r /= 64;
        const int kb = r % it.nkb; r /= it.nkb;
        const int chunk = (int)r;
        const int o = chunk * nc * 16 + nc * 4 * (m >> 2) + 4 * ct + (m & 3);
        const int k = kb * KB + q * EPL + j;
        float v = 0.f;
        if (o < O && k < K) {
            const unsigned mask = g_cls_masks[it.cls_kind].m[slot];
            for (int t = 0; t < 27; ++t)
                if ((mask >> t) & 1u) v += dgrad ? w[((size_t)t * cout_m + k) * cin_m + o] : w[((size_t)t * cout_m + o) * cin_m + k];
        }
        return v;
    }
    const int taps = it.taps;
    const int tap = r % taps; r /= taps;
    const int kb = r % it.nkb; r /= it.nkb;
    const int chunk = (int)r;
    const int o = chunk * nc * 16 + nc * 4 * (m >> 2) + 4 * ct + (m & 3);
    const int k = kb * KB + q * EPL + j;
    if (!(o < O && k < K)) return 0.f;
    return dgrad ? w[((size_t)(taps - 1 - tap) * cout_m + k) * cin_m + o] : w[((size_t)tap * cout_m + o) * cin_m + k];
}

// one block = one chunk (a whole number of [64 lanes][EPL] fragments): the slow coordinates (cout tile, tap, K-block, chunk) are
// block-uniform per fragment, only (lane, j) vary over the threads
template <typename T>
__global__ void __launch_bounds__(256) pack_many_kernel(const vdm_pack_item* __restrict__ items, const vdm_pack_chunk* __restrict__ chunks) {
    constexpr int EPL = DT<T>::EPL, FRAG = 64 * EPL;
    const vdm_pack_chunk c = chunks[blockIdx.x];
    const vdm_pack_item it = items[c.item];
    const float* w = it.w_master;
    T* out = reinterpret_cast<T*>(it.w_packed);
    const int j = threadIdx.x % EPL;
    for (long long f = c.first; f < c.first + c.count; f += FRAG) {          // (first and count are multiples of FRAG)
        const size_t r = (size_t)(f / FRAG);
#pragma unroll
        for (int u = 0; u < FRAG / 256; ++u) {
            const int e = threadIdx.x + u * 256;
            st_packed_w<T>(out, (size_t)(f + e), pack_value<T>(it, w, r, e / EPL, j));
        }
    }
}

// one item (kernel argument: no device-side table) through the same pack_value - vdm_conv_pack_weights
template <typename T>
__global__ void pack_item_kernel(const vdm_pack_item it) {
    constexpr int EPL = DT<T>::EPL;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)it.elems; i += (size_t)gridDim.x * blockDim.x)
        st_packed_w<T>(reinterpret_cast<T*>(it.w_packed), i, pack_value<T>(it, it.w_master, i / (64 * EPL), (int)(i / EPL % 64), (int)(i % EPL)));
}

extern "C" size_t vdm_conv_packed_bytes(const vdm_conv_desc* d, int pack_mode) {
    return validate(d) == VDM_OK ? plan_of(d, pack_mode == VDM_PACK_DGRAD).packed_bytes : 0;
}

extern "C" int vdm_conv_pack_plan(const vdm_conv_desc* d, int pack_mode, const float* w_master, void* w_packed, vdm_pack_item* item) {
    int e = validate(d);
    if (e) return e;
    VDM_REQUIRE(item && w_master && w_packed, "conv_pack_plan: NULL pointer");
    VDM_REQUIRE(pack_mode == VDM_PACK_FWD || pack_mode == VDM_PACK_DGRAD, "conv_pack_plan: bad mode %d", pack_mode);
    const Plan p = plan_of(d, pack_mode == VDM_PACK_DGRAD);
    item->w_master = w_master; item->w_packed = w_packed;
    item->taps = p.taps; item->cout = d->cout; item->cin = d->cin; item->nc = p.nc; item->nchunks = p.nchunks; item->nkb = p.nkb;
    item->dgrad = pack_mode == VDM_PACK_DGRAD;
    item->variant = p.layout; item->cls_kind = p.cls_kind;
    item->dtype = d->dtype;
    item->elems = (long long)(p.packed_bytes / (d->dtype == VDM_F32 ? 4 : 2));
    return VDM_OK;
}

// the class masks pack_value reads: uploaded once per device ordinal (the symbol lives in each device's copy of the module)
static int upload_cls_masks() {
    static unsigned long long masks_up = 0;
    const int dev = current_device();
    if (dev < 64 && ((masks_up >> dev) & 1ull)) return VDM_OK;
    ClsMasks h[3];
    ClsTable tab;
    for (int k = 0; k < 3; ++k) build_cls(k, tab, h[k]);
    int e = check_hip(hipMemcpyToSymbol(HIP_SYMBOL(g_cls_masks), h, sizeof(h)), "hipMemcpyToSymbol(g_cls_masks)");
    if (!e && dev < 64) masks_up |= 1ull << dev;
    return e;
}

extern "C" int vdm_conv_pack_weights(const vdm_conv_desc* d, int pack_mode, const float* w_master, void* w_packed, void* stream) {
    vdm_pack_item it;
    int e = vdm_conv_pack_plan(d, pack_mode, w_master, w_packed, &it);
    if (!e && it.variant == VDM_CONV_VARIANT_CLASS) e = upload_cls_masks();
    if (e) return e;
    const unsigned grid = (unsigned)((it.elems + 255) / 256 < 2048 ? (it.elems + 255) / 256 : 2048);
    if (d->dtype == VDM_F32)
        hipLaunchKernelGGL(pack_item_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, it);
    else
        hipLaunchKernelGGL(pack_item_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, it);
    VDM_LAUNCH_CHECK("pack_item_kernel");
    return VDM_OK;
}

extern "C" int vdm_conv_pack_many(const vdm_pack_item* items_dev, const vdm_pack_chunk* chunks_dev, int nchunks, int dtype, void* stream) {
    VDM_REQUIRE(items_dev && chunks_dev && nchunks > 0, "conv_pack_many: empty work list");
    VDM_REQUIRE(dtype == VDM_F32 || dtype == VDM_BF16, "conv_pack_many: bad dtype %d", dtype);
    int e = upload_cls_masks();
    if (e) return e;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VDM_F32)
        hipLaunchKernelGGL(pack_many_kernel<float>, dim3(nchunks), dim3(256), 0, s, items_dev, chunks_dev);
    else
        hipLaunchKernelGGL(pack_many_kernel<bf16_t>, dim3(nchunks), dim3(256), 0, s, items_dev, chunks_dev);
    VDM_LAUNCH_CHECK("pack_many_kernel");
    return VDM_OK;
}

// plan -> kernel arguments (either direction: a dgrad is a stride-1 conv on the output grid, where fill_dims gives I == S == D)
static ConvArgs conv_args(const vdm_conv_desc* d, const Plan& p) {
    ConvArgs a{};
    fill_dims(a, d);
    a.Cin = p.K; a.CinStride = cpad(p.K, d->dtype); a.Cout = p.O;
    a.nchunks = p.nchunks; a.nkb = p.nkb;
    return a;
}

extern "C" int vdm_conv_gn_tiles(const vdm_conv_desc* d) {
    return validate(d) == VDM_OK ? plan_of(d, 0).tiles : 0;       // (the up-sampling conv has one slot per coarse tile and class)
}

extern "C" int vdm_conv_fwd(const vdm_conv_desc* d, const void* x, const void* w_packed, const float* bias, const float* nbias,
                            int64_t nbias_stride, const void* residual, void* out, float* gn_partials, void* stream) {
    int e = validate(d);
    if (e) return e;
    VDM_REQUIRE(x && w_packed && out, "conv_fwd: NULL pointer");
    const Plan p = plan_of(d, 0);
    if (p.family == VDM_CONV_VARIANT_CLASS) {
        VDM_REQUIRE(!nbias && !d->out_f32, "conv_fwd: the up-sampling conv takes no per-sample bias / fp32 output");
        return run_cls(d, p, x, w_packed, bias, residual, out, (hipStream_t)stream, gn_partials);
    }
    ConvArgs a = conv_args(d, p);
    a.x = x; a.w = w_packed; a.bias = bias; a.nbias = nbias; a.nbias_stride = nbias_stride; a.res = residual; a.out = out;
    a.gnp = gn_partials;
    return launch_fwd(a, p, (hipStream_t)stream);
}

extern "C" int vdm_conv_dgrad(const vdm_conv_desc* d, const void* dout, const void* w_packed_dgrad, const void* residual, void* dx,
                              void* stream) {
    int e = validate(d);
    if (e) return e;
    VDM_REQUIRE(dout && w_packed_dgrad && dx, "conv_dgrad: NULL pointer");
    const Plan p = plan_of(d, 1);
    // up-sampling conv: dout is (od,oh,ow), dx is the coarse input (od/2,..);  stride-2 conv: dout is (od,oh,ow), dx is (2od,..)
    if (p.family == VDM_CONV_VARIANT_CLASS) return run_cls(d, p, dout, w_packed_dgrad, nullptr, residual, dx, (hipStream_t)stream);
    ConvArgs a = conv_args(d, p);
    a.x = dout; a.w = w_packed_dgrad; a.res = residual; a.out = dx;
    return launch_fwd(a, p, (hipStream_t)stream);
}

extern "C" int vdm_conv_dgrad_gn_tiles(const vdm_conv_desc* d) {
    if (validate(d) != VDM_OK || d->ksize != 3 || d->stride != 1 || d->upsample) return 0;
    return plan_of(d, 1).tiles;
}

extern "C" int vdm_conv_dgrad_gn(const vdm_conv_desc* d, const void* dout, const void* w_packed_dgrad, void* dyh, const vdm_gn_fold* f,
                                 void* stream) {
    int e = validate(d);
    if (e) return e;
    VDM_REQUIRE(dout && w_packed_dgrad && dyh && f, "conv_dgrad_gn: NULL pointer");
    VDM_REQUIRE(d->ksize == 3 && d->stride == 1 && !d->upsample, "conv_dgrad_gn: only the 3x3x3 stride-1 conv feeds a GroupNorm backward");
    VDM_REQUIRE(f->x1 && f->stats && f->gamma && f->beta && f->partials && f->groups > 0, "conv_dgrad_gn: NULL pointer in the fold");
    const int C = d->cin;
    const Plan p = plan_of(d, 1);
    VDM_REQUIRE(f->c1 + f->c2 == C && (f->c2 == 0 || f->x2), "conv_dgrad_gn: c1 + c2 must equal the conv's input channels (%d)", C);
    VDM_REQUIRE(C % f->groups == 0 && C % (p.nc * 4) == 0 && C % epl_of(d->dtype) == 0, "conv_dgrad_gn: channel count %d not supported", C);
    VDM_REQUIRE(f->c2 == 0 || f->c1 % (p.nc * 4) == 0, "conv_dgrad_gn: a lane's %d channels would straddle the concat boundary", p.nc * 4);
    ConvArgs a = conv_args(d, p);
    a.x = dout; a.w = w_packed_dgrad; a.out = dyh; a.gnp = f->partials;
    a.gx1 = f->x1; a.gx2 = f->x2; a.gc1 = f->c1; a.gc2 = f->c2; a.gG = f->groups;
    a.gstats = f->stats; a.ggamma = f->gamma; a.gbeta = f->beta; a.gmask = f->keep_mask;
    a.geps = f->eps; a.ginv_keep = f->keep_mask ? f->inv_keep : 1.0f;
    a.gcnt = (float)((double)d->od * d->oh * d->ow * (C / f->groups));
    return launch_fwd_gnb(a, p, (hipStream_t)stream);
}

extern "C" int vdm_conv_kernel_variant(const vdm_conv_desc* d, int dgrad) {
    return validate(d) ? -1 : plan_of(d, dgrad).family;
}

extern "C" int vdm_conv_plan(const vdm_conv_desc* d, int dgrad, vdm_conv_plan_info* out) {
    int e = validate(d);
    if (e) return e;
    VDM_REQUIRE(out, "conv_plan: NULL pointer");
    const Plan p = plan_of(d, dgrad != 0);
    const long long nwg = plan_workgroups(p);
    out->family = p.family; out->layout = p.layout; out->cls_kind = p.cls_kind;
    out->nc = p.nc; out->nchunks = p.nchunks; out->nkb = p.nkb;
    out->tz = p.tz; out->ty = p.ty;
    out->roll = p.roll; out->nseg = p.nseg; out->zsteps = p.zsteps;
    out->tiles = p.tiles;
    out->workgroups = (int32_t)(nwg < 0x7fffffffLL ? nwg : 0x7fffffffLL);
    out->reserved = 0;
    out->packed_bytes = p.packed_bytes;
    // the descriptor-level refusals of vdm_conv_fwd (launch_fwd, the class branch of vdm_conv_fwd)
    if (nwg > 0x7fffffffLL) { set_error("conv: grid too large"); return VDM_ERR_ARG; }
    if (p.out_f32 && p.family == VDM_CONV_VARIANT_CLASS) {
        set_error("conv_fwd: the up-sampling conv takes no per-sample bias / fp32 output");
        return VDM_ERR_ARG;
    }
    if (p.out_f32 && p.dtype == VDM_BF16 && !(p.ks == 3 && p.stride == 1 && !p.ups && p.nc == 1)) {
        set_error("conv: out_f32 with bf16 input is only built for ksize 3, stride 1, cout <= 16");
        return VDM_ERR_UNSUPPORTED;
    }
    return VDM_OK;
}

// largest workspace over the (want_bias, accumulate) combinations: they change which kernel serves a descriptor
extern "C" size_t vdm_conv_wgrad_workspace_bytes(const vdm_conv_desc* d) {
    if (validate(d) != VDM_OK) return 0;
    size_t need = 0;
    for (int k = 0; k < 4; ++k) need = std::max(need, plan_wgrad(d, (k & 1) != 0, (k & 2) != 0).workspace_bytes);
    return need;
}

extern "C" int vdm_conv_wgrad_plan(const vdm_conv_desc* d, int want_bias, int accumulate, vdm_wgrad_plan_info* out) {
    int e = validate(d);
    if (e) return e;
    VDM_REQUIRE(out, "conv_wgrad_plan: NULL pointer");
    const WgradPlan p = plan_wgrad(d, want_bias != 0, accumulate != 0);
    out->kernel = p.kernel; out->tz = p.tz; out->ty = p.ty;
    out->workgroups = p.grid; out->tiles = p.ntiles; out->P = p.P;
    out->workspace_bytes = p.workspace_bytes;
    if (want_bias && d->ksize == 1) { set_error("conv_wgrad: fused bias gradient is only built for ksize 3"); return VDM_ERR_UNSUPPORTED; }
    return VDM_OK;
}

extern "C" int vdm_conv_wgrad(const vdm_conv_desc* d, const void* x, const void* dout, float* dw, float* dbias, int accumulate,
                              void* workspace, size_t workspace_bytes, void* stream) {
    int e = validate(d);
    if (e) return e;
    VDM_REQUIRE(x && dout && dw && workspace, "conv_wgrad: NULL pointer");
    const WgradPlan p = plan_wgrad(d, dbias != nullptr, accumulate != 0);
    hipStream_t s = (hipStream_t)stream;
    if (p.kernel == VDM_WGRAD_THIN_IN || p.kernel == VDM_WGRAD_THIN_OUT) {
        const bool in = p.kernel == VDM_WGRAD_THIN_IN;       // the dense side is dout (conv_in) or x (conv_out)
        ThinArgs a{};
        a.dense = (const bf16_t*)(in ? dout : x);
        a.N = d->n; a.Dz = d->od; a.Dy = d->oh; a.Dx = d->ow; a.C = in ? d->cout : d->cin; a.circular = d->pad_mode == VDM_PAD_CIRCULAR;
        return launch_wgrad_thin(a, false, p, in ? x : dout, d->cin, dw, dbias, workspace, workspace_bytes, s);
    }
    WgradArgs w{};
    fill_dims(w.c, d);
    w.c.x = x;
    w.c.Cin = d->cin; w.c.CinStride = cpad(d->cin, d->dtype); w.c.Cout = d->cout;
    w.dout = dout; w.dout_stride = cpad(d->cout, d->dtype);
    w.slabs = (float*)workspace;
    w.ncb = p.ncb; w.nkb = p.nkb;
    return launch_wgrad_any(w, p, dw, dbias, accumulate, workspace_bytes, d->dtype, s);
}


#ifdef VDM_TIMELINE
namespace vdm { unsigned long long* g_timeline_stamps = nullptr; }
// diagnostic build only (make timeline): every later conv_fwd_kernel launch writes [workgroup][wave][8] stamps to `buf`
extern "C" int vdm_debug_set_stamps(void* buf) {
    vdm::g_timeline_stamps = (unsigned long long*)buf;
    return VDM_OK;
}
#endif
