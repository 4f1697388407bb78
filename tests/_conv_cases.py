"""The case table of the forward / input-gradient conv kernel checks: tests/test_conv_kernels_gpu.py runs the cases on the device,
tests/test_conv_cpu.py confirms with the host-only plan query (vdm_conv_plan) that every case reaches the kernel, tile and segmenting it
names.  The plan depends on the CU count; without a device the library plans for 256 CUs, the MI355X's count, so both see the same plans
(the device test asserts the plan again before it launches)."""
import ctypes
from collections import namedtuple

import torch

import _conv_ref as R

BF, F32 = torch.bfloat16, torch.float32

# grid = (D, H, W) of the conv's OUTPUT; direction "fwd" (vdm_conv_fwd) or "dgrad" (vdm_conv_dgrad of the same conv);
# family = VDM_CONV_VARIANT_* the case is there for; fields = vdm_conv_plan_info values it is there for (cls_kind by name)
Case = namedtuple("Case", "name dtype cin cout n grid ks stride ups circ out_f32 direction family fields")
FAMILIES = ("GENERIC", "CLASS", "KPACK", "SPLIT", "KSPLIT")
CLS_KINDS = ("UP_FWD", "UP_DGRAD", "S2_DGRAD")


def C(name, dtype, cin, cout, n, grid, direction, family, ks=3, stride=1, ups=0, circ=False, out_f32=False, **fields):
    return Case(name, dtype, cin, cout, n, grid, ks, stride, ups, circ, out_f32, direction, family, fields)


def both(name, dtype, cin, cout, n, grid, fwd, dgrad, **kw):
    """A forward and a dgrad case of the same conv; fwd / dgrad = (family, fields)."""
    return [C(name + "_fwd", dtype, cin, cout, n, grid, "fwd", fwd[0], **kw, **fwd[1]),
            C(name + "_dgrad", dtype, cin, cout, n, grid, "dgrad", dgrad[0], **kw, **dgrad[1])]


def same(name, dtype, cin, cout, n, grid, family, kw=None, **fields):
    return both(name, dtype, cin, cout, n, grid, (family, fields), (family, fields), **(kw or {}))


def one(name, dtype, cin, cout, n, grid, direction, family, kw=None, **fields):
    return [C(f"{name}_{direction}", dtype, cin, cout, n, grid, direction, family, **(kw or {}), **fields)]


def zc(fn, name, *a, kw=None, **k):
    """The case(s) with zero and with circular padding."""
    return fn(name, *a, kw=dict(kw or {}), **k) + fn(name + "_circ", *a, kw=dict(kw or {}, circ=True), **k)


S2F, S2D = ("GENERIC", dict(tz=2, ty=4)), ("CLASS", dict(cls_kind="S2_DGRAD"))
UPF, UPD = ("CLASS", dict(cls_kind="UP_FWD")), ("CLASS", dict(cls_kind="UP_DGRAD"))


def s2(name, dtype, cin, cout, n, grid, circ=False, **nc):
    fw = {k[4:]: v for k, v in nc.items() if k.startswith("fwd_")}
    dg = {k[6:]: v for k, v in nc.items() if k.startswith("dgrad_")}
    return both(name, dtype, cin, cout, n, grid, (S2F[0], dict(S2F[1], **fw)), (S2D[0], dict(S2D[1], **dg)), stride=2, circ=circ)


def up(name, dtype, cin, cout, n, grid, circ=False, **nc):
    fw = {k[4:]: v for k, v in nc.items() if k.startswith("fwd_")}
    dg = {k[6:]: v for k, v in nc.items() if k.startswith("dgrad_")}
    return both(name, dtype, cin, cout, n, grid, (UPF[0], dict(UPF[1], **fw)), (UPD[0], dict(UPD[1], **dg)), ups=1, circ=circ)


CASES = [
    # ---- bf16 3x3x3 stride 1, 32 -> 32 (NC = 2, one K-block): the generic kernel at its small tiles, then the rolling z window
    *zc(same, "g_1x4_ragged", BF, 32, 32, 1, (3, 5, 18), "GENERIC", tz=1, ty=4, roll=0),            # ragged in y and x
    *zc(same, "g_one_voxel", BF, 32, 32, 1, (1, 1, 1), "GENERIC", tiles=1),                         # every tap is padding / wraps onto itself
    *same("g_two_samples", BF, 32, 32, 2, (3, 5, 18), "GENERIC", tz=1, ty=4),                       # no halo may leak across the sample boundary
    *same("g_1x8", BF, 32, 32, 2, (9, 33, 40), "GENERIC", tz=1, ty=8, roll=0),
    *same("g_2x8", BF, 32, 32, 3, (10, 41, 40), "GENERIC", tz=2, ty=8, roll=0),
    *zc(same, "roll_equal_segments", BF, 32, 32, 4, (29, 57, 17), "GENERIC", tz=4, ty=8, roll=1, nseg=4, zsteps=2),   # ragged in z, y and x
    *same("roll_unequal_segments", BF, 32, 32, 4, (26, 73, 17), "GENERIC", tz=4, ty=8, roll=1, nseg=3, zsteps=3),     # 7 z tiles: 3, 3, 1 steps
    C("roll_partial_kblock_fwd", BF, 24, 32, 4, (29, 57, 17), "fwd", "GENERIC", tz=4, ty=8, roll=1, nkb=1),
    # ---- 64-channel chunks (NC = 4): the 4x8x16 tile never rolls; small grids take half chunks (SPLIT)
    *same("g_nc4_4x8", BF, 64, 64, 4, (29, 57, 17), "GENERIC", tz=4, ty=8, nkb=2, nc=4, roll=0),
    *same("split_1x4", BF, 64, 64, 1, (3, 5, 18), "SPLIT", tz=1, ty=4),
    *same("split_1x8", BF, 64, 64, 2, (9, 33, 40), "SPLIT", tz=1, ty=8),
    *same("split_2x8", BF, 64, 64, 3, (11, 41, 40), "SPLIT", tz=2, ty=8),
    *both("split_3kb", BF, 96, 64, 1, (3, 5, 18), ("SPLIT", dict(nkb=3)), ("GENERIC", dict(nc=4, nchunks=2, nkb=2))),   # dgrad: a partial chunk
    *same("g_nc4_partial_48", BF, 48, 48, 1, (3, 5, 18), "GENERIC", nc=4, nchunks=1, nkb=2),        # partial chunk and partial K-block
    *same("g_nc4_1x8", BF, 48, 48, 2, (9, 33, 40), "GENERIC", nc=4, tz=1, ty=8),                    # the small tiles of a chunk that SPLIT does not take
    *same("g_nc4_2x8", BF, 48, 48, 3, (11, 41, 40), "GENERIC", nc=4, tz=2, ty=8),
    *both("g_partial_24_40", BF, 24, 40, 1, (3, 5, 18), ("GENERIC", dict(nc=4, nkb=1)), ("GENERIC", dict(nc=2, nkb=2))),
    # ---- the K-split kernel of the deepest level
    *same("ksplit_ty4", BF, 128, 128, 1, (3, 9, 40), "KSPLIT", tz=1, ty=4, nkb=4, nchunks=2),
    C("ksplit_5kb_circ_fwd", BF, 160, 128, 2, (3, 6, 20), "fwd", "KSPLIT", circ=True, nkb=5),       # K-blocks per wave: 2, 1, 1, 1
    *same("ksplit_ty8", BF, 128, 128, 2, (5, 33, 40), "KSPLIT", tz=1, ty=8),
    C("ksplit_8kb_fwd", BF, 256, 128, 1, (5, 33, 40), "fwd", "KSPLIT", nkb=8, ty=4),
    # ---- <= 8 reduction channels: the tap-packed kernel (NC = 2 and 1), as a forward and as conv_out's input gradient
    *zc(one, "kpack_2_32", BF, 2, 32, 1, (5, 9, 18), "fwd", "KPACK", nc=2),
    *zc(one, "kpack_3_16", BF, 3, 16, 1, (5, 9, 18), "fwd", "KPACK", nc=1),
    *zc(one, "kpack_8_16", BF, 8, 16, 1, (5, 9, 18), "fwd", "KPACK", nc=1),
    C("kpack_conv_out_dgrad", BF, 32, 1, 1, (5, 9, 18), "dgrad", "KPACK", nc=2),
    # ---- one 16-channel output tile (NC = 1); conv_in's input gradient; conv_out with its fp32 output
    *same("g_nc1", BF, 16, 16, 1, (5, 9, 18), "GENERIC", nc=1),
    C("g_conv_in_dgrad", BF, 2, 32, 1, (5, 9, 18), "dgrad", "GENERIC", nc=1),
    C("g_conv_out_f32_fwd", BF, 32, 1, 1, (5, 9, 18), "fwd", "GENERIC", out_f32=True, nc=1),
    # ---- fp32 storage (bf16 pipe with three MFMAs per product, or the exact fp32 MFMA): 16-channel K-blocks
    *same("f32_32_32_circ", F32, 32, 32, 1, (3, 9, 18), "GENERIC", kw=dict(circ=True), nkb=2),
    *same("f32_20_24_circ", F32, 20, 24, 1, (3, 9, 18), "GENERIC", kw=dict(circ=True), nkb=2),
    C("f32_2x8_fwd", F32, 64, 64, 2, (9, 57, 40), "fwd", "GENERIC", tz=2, ty=8, nkb=4),
    # ---- ksize 1
    *same("k1_64_32", BF, 64, 32, 2, (6, 9, 20), "GENERIC", kw=dict(ks=1), tz=4, ty=8),
    *same("k1_32_128", BF, 32, 128, 2, (6, 9, 20), "GENERIC", kw=dict(ks=1), tz=4, ty=8),
    *same("k1_64_32_f32", F32, 64, 32, 2, (6, 9, 20), "GENERIC", kw=dict(ks=1), tz=4, ty=8),
    # ---- stride 2 (output grids): the 2x4x16 forward tile; its input gradient is the class kernel with 1 / 2 / 4 / 8 taps per class
    *s2("s2_32_64", BF, 32, 64, 1, (3, 5, 10), dgrad_nc=2),
    *s2("s2_32_64_circ", BF, 32, 64, 1, (3, 5, 10), circ=True),
    *s2("s2_32_64_f32", F32, 32, 64, 1, (3, 5, 10)),
    *s2("s2_32_64_circ_f32", F32, 32, 64, 1, (3, 5, 10), circ=True),
    *s2("s2_64_64_1x1x2_circ", BF, 64, 64, 1, (1, 1, 2), circ=True, dgrad_nc=4),                     # input 2 x 2 x 4: smaller than the halo
    *s2("s2_16_32", BF, 16, 32, 1, (3, 5, 10), dgrad_nc=1),
    # ---- up-sampling conv (output grids): the class kernels on the coarse grid, NC = 1 / 2 / 4 in both directions
    *up("ups_32_16", BF, 32, 16, 1, (6, 10, 24), fwd_nc=1, dgrad_nc=2),                              # coarse grid 3 x 5 x 12: ragged
    *up("ups_32_16_circ", BF, 32, 16, 1, (6, 10, 24), circ=True),
    *up("ups_64_32", BF, 64, 32, 1, (6, 10, 24), fwd_nc=2, dgrad_nc=4),
    *up("ups_64_32_circ", BF, 64, 32, 1, (6, 10, 24), circ=True),
    *up("ups_128_64", BF, 128, 64, 1, (6, 10, 36), fwd_nc=4, fwd_nkb=4, dgrad_nchunks=2),            # coarse x 18: a second x tile
    *up("ups_32_32_2x2x2_circ", BF, 32, 32, 2, (2, 2, 2), circ=True),                                # coarse grid 1 x 1 x 1
    *up("ups_64_32_f32", F32, 64, 32, 1, (6, 10, 24)),
    *up("ups_16_32", BF, 16, 32, 1, (6, 10, 24), dgrad_nc=1),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# check B: one case per kernel and tile, at A's shapes
B_CASES = ["g_1x4_ragged_circ_fwd", "g_1x8_fwd", "g_2x8_dgrad", "roll_equal_segments_fwd", "roll_unequal_segments_dgrad", "g_nc4_4x8_fwd",
           "split_1x4_fwd", "split_1x8_dgrad", "split_2x8_fwd", "g_partial_24_40_dgrad", "ksplit_ty4_fwd", "ksplit_5kb_circ_fwd",
           "ksplit_ty8_dgrad", "kpack_2_32_fwd", "kpack_3_16_circ_fwd", "kpack_conv_out_dgrad", "g_nc1_fwd", "g_conv_out_f32_fwd",
           "f32_20_24_circ_fwd", "f32_20_24_circ_dgrad", "k1_64_32_fwd", "k1_64_32_f32_dgrad", "s2_32_64_fwd", "s2_32_64_f32_fwd",
           "s2_32_64_dgrad", "s2_32_64_f32_dgrad", "ups_32_16_fwd", "ups_64_32_fwd", "ups_128_64_fwd", "ups_64_32_f32_fwd",
           "ups_64_32_dgrad", "ups_16_32_dgrad", "ups_64_32_f32_dgrad"]
# forward cases that also run with gn_partials requested (check A): one per family
GN_CASES = ["g_1x4_ragged_fwd", "roll_equal_segments_fwd", "split_1x4_fwd", "ksplit_ty4_fwd", "kpack_2_32_fwd", "ups_64_32_fwd"]


def K(c):
    """Reduction channels of the launch."""
    return c.cout if c.direction == "dgrad" else c.cin


def O(c):
    """Output channels of the launch."""
    return c.cin if c.direction == "dgrad" else c.cout


def terms(c):
    """The longest sum of products one output value is: taps x reduction channels (the up-sampling conv's input gradient sums the 2x2x2
    fine voxels of a source voxel), plus the epilogue terms (each below 9)."""
    return c.ks ** 3 * K(c) * (8 if c.ups and c.direction == "dgrad" else 1) + 3


def ishape(c):
    """[N, Di, Hi, Wi] of the conv's input (= of dx)."""
    return R.input_shape(c.n, c.grid, c.stride, c.ups)


def oshape(c):
    return (c.n,) + tuple(c.grid)


def in_shape(c):
    """Shape of the tensor the launch stages (x, or dout)."""
    return (oshape(c) + (c.cout,)) if c.direction == "dgrad" else (ishape(c) + (c.cin,))


def out_shape(c):
    return (ishape(c) + (c.cin,)) if c.direction == "dgrad" else (oshape(c) + (c.cout,))


def out_dtype(c):
    return F32 if (c.out_f32 and c.direction == "fwd") else c.dtype


def desc_of(c):
    from vdm4cdm_amd import _lib
    D, H, W = c.grid
    return _lib.ConvDesc(n=c.n, od=D, oh=H, ow=W, cin=c.cin, cout=c.cout, ksize=c.ks, stride=c.stride, upsample=c.ups,
                         pad_mode=_lib.PAD_CIRCULAR if c.circ else _lib.PAD_ZEROS, dtype=_lib.VDM_BF16 if c.dtype == BF else _lib.VDM_F32,
                         out_f32=int(c.out_f32))


def plan_of(c):
    """(descriptor, vdm_conv_plan_info) of the launch the case makes: host only."""
    from vdm4cdm_amd import _lib
    d = desc_of(c)
    info = _lib.ConvPlanInfo()
    st = _lib.lib().vdm_conv_plan(d, int(c.direction == "dgrad"), ctypes.byref(info))
    assert st == 0, _lib.lib().vdm_last_error()
    return d, info


def family_of(info):
    return FAMILIES[info.family]


def cls_kind_of(info):
    return CLS_KINDS[info.cls_kind] if family_of(info) == "CLASS" else None


def assert_plan(c, info):
    """The case reaches the kernel it names, with the plan fields it is there for."""
    assert family_of(info) == c.family, f"{c.name}: the plan runs {family_of(info)}, the case is there for {c.family}"
    for k, v in c.fields.items():
        got = cls_kind_of(info) if k == "cls_kind" else getattr(info, k)
        assert got == v, f"{c.name}: plan {k} = {got}, expected {v}"


def epilogue_terms(c):
    """Additions of the full-epilogue variant: bias and per-sample bias (formed, then added) and the residual; the up-sampling conv takes
    no per-sample bias; a dgrad only the residual."""
    if c.direction == "dgrad":
        return 1
    return 2 if c.ups else 3


def depth(c, info, fp32_exact):
    return R.depth(family_of(info), cls_kind_of(info), c.dtype == BF, fp32_exact, c.ks, info.nkb, epilogue_terms(c))


def ref(c, xin, w, bias=None, nbias=None, res=None, dtype=torch.float64, want_abs=True):
    """The reference of the case's launch: xin is x (fwd) or dout (dgrad)."""
    if c.direction == "dgrad":
        return R.ref_dgrad(xin, w, c.ks, c.stride, c.ups, c.circ, res=res, dtype=dtype, want_abs=want_abs)
    return R.ref_fwd(xin, w, c.ks, c.stride, c.ups, c.circ, bias=bias, nbias=nbias, res=res, dtype=dtype, want_abs=want_abs)


NBIAS_STRIDE_EXTRA = 5          # the per-sample bias is a column block of a wider [n][sum cout] table


def epilogue_operands(c, seed, real):
    """(bias, nbias, res) of the full-epilogue variant (CPU, fp32; res in the storage type's values).  Check A: integers (bias, nbias in
    [-8, 8], res in {-2..3}); check B: reals, res rounded to the storage type."""
    g = torch.Generator().manual_seed(seed)
    co = O(c)
    if real:
        bias, nbias = torch.randn(co, generator=g), torch.randn(c.n, co, generator=g)
        res = torch.randn(out_shape(c), generator=g).to(c.dtype).float()
    else:
        bias = torch.randint(-8, 9, (co,), generator=g, dtype=torch.int8).float()
        nbias = torch.randint(-8, 9, (c.n, co), generator=g, dtype=torch.int8).float()
        res = torch.randint(-2, 4, out_shape(c), generator=g, dtype=torch.int8).float()
    if c.direction == "dgrad":
        return None, None, res
    return bias, (None if c.ups else nbias), res


def real_operands(c, seed):
    """check B: randn rounded to the storage type; the staged tensor offset by 0.3 so that the sums do not centre on zero; master weights
    scaled to keep the outputs of order one."""
    g = torch.Generator().manual_seed(seed)
    xin = (torch.randn(in_shape(c), generator=g) + 0.3).to(c.dtype).float()
    w = (torch.randn((c.ks ** 3, c.cout, c.cin), generator=g) * (c.ks ** 3 * K(c)) ** -0.5).to(c.dtype).float()
    return xin, w
