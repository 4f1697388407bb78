"""The case table of the weight-gradient kernel checks: tests/test_wgrad_kernels_gpu.py runs the cases on the device,
tests/test_wgrad_cpu.py confirms with the host-only plan query (vdm_conv_wgrad_plan) that every case reaches the kernel it names."""
import ctypes
from collections import namedtuple

import torch

import _wgrad_ref as R

BF, F32 = torch.bfloat16, torch.float32

# grid = (D, H, W) of the OUTPUT (= of dout); fields = plan fields the case is there for (vdm_wgrad_plan_info: P, tiles, workgroups, tz, ty)
Case = namedtuple("Case", "name dtype cin cout n grid ks stride ups circ bias acc kernel fields")


def C(name, dtype, cin, cout, n, grid, kernel, ks=3, stride=1, ups=0, circ=False, bias=True, acc=False, **fields):
    return Case(name, dtype, cin, cout, n, grid, ks, stride, ups, circ, bias and ks == 3, acc, kernel, fields)


def _both(name, *a, **k):
    return [C(name + "_bf16", BF, *a, **k), C(name + "_f32", F32, *a, **k)]


# ------------------------------------------------------------------------------------------------ the thin-side grids
THIN_GRIDS = {
    "5x7x33": (1, (5, 7, 33), False),            # one voxel into a second x chunk
    "1x1x17_circ": (1, (1, 1, 17), True),        # the smallest circular width the kernel takes; z and y wrap onto themselves
    "3x5x31_circ": (1, (3, 5, 31), True),        # circular, one short of a chunk
    "3x5x32_circ": (1, (3, 5, 32), True),        # circular, exactly a chunk
    "4x4x70_circ": (2, (4, 4, 70), True),        # three x chunks, two samples
    "16x33x40": (2, (16, 33, 40), False),        # 2112 chunks for 512 workgroups x 4 waves: 64 waves take a second chunk
}
# (cin, cout, grid): every grid twice, every dense width four times, both thin widths on every second case
THIN_IN = [(1, 16, "5x7x33"), (2, 32, "5x7x33"), (2, 64, "1x1x17_circ"), (1, 32, "1x1x17_circ"), (1, 64, "3x5x31_circ"),
           (2, 16, "3x5x31_circ"), (2, 32, "3x5x32_circ"), (1, 64, "3x5x32_circ"), (1, 32, "4x4x70_circ"), (2, 16, "4x4x70_circ"),
           (2, 32, "16x33x40"), (1, 64, "16x33x40")]
THIN_OUT = [(16, "5x7x33"), (32, "1x1x17_circ"), (64, "3x5x31_circ"), (16, "3x5x32_circ"), (32, "4x4x70_circ"), (64, "16x33x40"),
            (32, "16x33x40")]


def _thin_cases():
    out = []
    for i, (cin, cout, g) in enumerate(THIN_IN):
        n, grid, circ = THIN_GRIDS[g]
        fields = dict(P=512, workgroups=512) if g == "16x33x40" else {}
        out.append(C(f"thin_in_{cin}_{cout}_{g}", BF, cin, cout, n, grid, "THIN_IN", circ=circ, bias=(i != 3), **fields))      # one case without a bias
    for cin, g in THIN_OUT:
        n, grid, circ = THIN_GRIDS[g]
        out.append(C(f"thin_out_{cin}_{g}", BF, cin, 1, n, grid, "THIN_OUT", circ=circ, bias=False))
    return out


CASES = [
    # ---- bf16, 3x3x3, stride 1, 32 -> 32: the rows kernel with and without the rolling z window
    C("roll_half_ztile", BF, 32, 32, 1, (7, 9, 20), "ROWS_ROLL", P=8, tiles=8),                       # 4 columns x 2 segments x 2 steps; half a z tile, ragged y and x
    C("roll_unequal_segments", BF, 32, 32, 1, (9, 8, 16), "ROWS_ROLL", P=2, tiles=2),                 # 5 z tiles: segments of 3 and 2 steps (odd step count)
    C("roll_two_samples_circ", BF, 32, 32, 2, (11, 9, 20), "ROWS_ROLL", circ=True, P=24, tiles=24),   # 8 columns x 3 segments
    C("roll_grouped_reduce", BF, 32, 32, 2, (16, 30, 40), "ROWS_ROLL", P=96, tiles=96),               # P > 32: grouped slab reduce
    C("rows_one_ztile", BF, 32, 32, 1, (2, 9, 20), "ROWS", P=4, tiles=4),                             # ntz = 1: the plain rows kernel
    C("rows_below_tile_circ", BF, 32, 32, 1, (2, 4, 6), "ROWS", circ=True, P=1, tiles=1),             # grid smaller than one tile and than the halo
    C("rows_1x1x1_circ", BF, 32, 32, 1, (1, 1, 1), "ROWS", circ=True, P=1, tiles=1),                  # every tap wraps onto the same voxel
    C("roll_acc", BF, 32, 32, 1, (7, 9, 20), "ROWS_ROLL", acc=True, P=8, tiles=8),
    C("rows_acc", BF, 32, 32, 1, (2, 9, 20), "ROWS", acc=True, P=4, tiles=4),
    # ---- other bf16 stride-1 shapes
    C("roll_256_two_columns", BF, 256, 256, 1, (7, 20, 40), "ROWS_ROLL", P=8, tiles=9, workgroups=512),   # 64 pairs x 8 workgroups, 9 columns: one walks two
    C("rows_256_scattered", BF, 256, 256, 1, (3, 20, 40), "ROWS", P=8, tiles=18, workgroups=512),         # 18 scattered tiles for 8 workgroups
    C("roll_48_96_circ", BF, 48, 96, 1, (5, 9, 20), "ROWS_ROLL", circ=True, P=4, tiles=4, workgroups=24), # partial channel blocks; one 3-step segment
    C("roll_24_40_circ", BF, 24, 40, 1, (5, 9, 20), "ROWS_ROLL", circ=True, P=4, tiles=4, workgroups=8),
    C("tapsplit_16_32", BF, 16, 32, 1, (5, 9, 20), "TAPSPLIT", tz=2, ty=8),                           # one real 16-channel tile of the input block
    C("tapsplit_8_32_circ", BF, 8, 32, 1, (5, 9, 20), "TAPSPLIT", circ=True, tz=2, ty=8),
    C("tapsplit_32_16", BF, 32, 16, 1, (5, 9, 20), "TAPSPLIT", tz=2, ty=8),                           # one real tile of the dOut block
    # ---- fp32: the tap-split kernel with 16-channel blocks
    C("f32_20_24_circ", F32, 20, 24, 1, (3, 9, 18), "TAPSPLIT", circ=True, tz=2, ty=8, P=8, workgroups=32),       # 2 x 2 blocks of 16 channels
    C("f32_32_32", F32, 32, 32, 2, (5, 9, 20), "TAPSPLIT", tz=2, ty=8),
    C("f32_20_24_circ_acc", F32, 20, 24, 1, (3, 9, 18), "TAPSPLIT", circ=True, acc=True, tz=2, ty=8),
    # ---- stride 2 (output grids)
    *_both("s2_32_64", 32, 64, 1, (3, 5, 10), "TAPSPLIT", stride=2, tz=1, ty=4),
    *_both("s2_32_64_circ", 32, 64, 1, (3, 5, 10), "TAPSPLIT", stride=2, circ=True, tz=1, ty=4),
    *_both("s2_64_64_1x1x2_circ", 64, 64, 1, (1, 1, 2), "TAPSPLIT", stride=2, circ=True, tz=1, ty=4),     # input 2 x 2 x 4: smaller than the halo
    C("s2_32_64_acc_bf16", BF, 32, 64, 1, (3, 5, 10), "TAPSPLIT", stride=2, acc=True, tz=1, ty=4),
    # ---- ksize 1: four slab slots per workgroup, no bias gradient
    *_both("k1_64_32", 64, 32, 2, (6, 9, 20), "TAPSPLIT", ks=1, tz=4, ty=8, P=16),                    # 16 x 4 slabs: grouped reduce
    *_both("k1_32_128", 32, 128, 2, (6, 9, 20), "TAPSPLIT", ks=1, tz=4, ty=8, P=16),
    C("k1_64_32_acc_bf16", BF, 64, 32, 2, (6, 9, 20), "TAPSPLIT", ks=1, acc=True, tz=4, ty=8, P=16),
    # ---- up-sampling conv (output grids): the parity-class kernel on the coarse grid
    *_both("ups_64_32", 64, 32, 1, (6, 10, 24), "CLASS", ups=1, tz=2, ty=8),                          # coarse grid 3 x 5 x 12: ragged
    *_both("ups_64_32_circ", 64, 32, 1, (6, 10, 24), "CLASS", ups=1, circ=True, tz=2, ty=8),
    *_both("ups_32_32_2x2x2_circ", 32, 32, 2, (2, 2, 2), "CLASS", ups=1, circ=True, tz=2, ty=8),      # coarse grid 1 x 1 x 1
    C("ups_64_32_acc_bf16", BF, 64, 32, 1, (6, 10, 24), "CLASS", ups=1, acc=True, tz=2, ty=8),
    # ---- the thin-side kernels and where their refusals land
    *_thin_cases(),
    C("thin_in_fallback_circ_ow16", BF, 2, 32, 1, (5, 7, 16), "TAPSPLIT", circ=True),                 # circular and 16 wide
    C("thin_in_fallback_acc", BF, 2, 32, 1, (5, 7, 33), "TAPSPLIT", acc=True),                        # the thin kernels only write
    C("thin_out_fallback_acc", BF, 32, 1, 1, (5, 7, 33), "TAPSPLIT", bias=False, acc=True),
    C("thin_out_fallback_bias", BF, 32, 1, 1, (5, 7, 33), "TAPSPLIT"),                                # cout = 1 with a bias gradient
    C("thin_in_fallback_2_48", BF, 2, 48, 1, (5, 7, 33), "TAPSPLIT"),                                 # no thin kernel for 48 dense channels
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# check B: one case per kernel, at A's shapes
B_CASES = ["roll_half_ztile", "roll_grouped_reduce", "rows_one_ztile", "rows_256_scattered", "tapsplit_16_32", "f32_20_24_circ",
           "s2_32_64_bf16", "s2_32_64_f32", "k1_64_32_bf16", "ups_64_32_bf16", "thin_in_1_16_5x7x33", "thin_in_2_32_16x33x40",
           "thin_out_32_4x4x70_circ"]


def terms(c):
    """The longest sum of products a case forms: the voxels of dout."""
    return c.n * c.grid[0] * c.grid[1] * c.grid[2]


def ishape(c):
    return R.input_shape(c.n, c.grid, c.stride, c.ups)


def conv_of(c):
    from vdm4cdm_amd import hip_ops as ops
    return ops.Conv(c.cin, c.cout, c.ks, stride=c.stride, upsample=c.ups, circular=c.circ)


def plan_of(c, conv=None):
    """(descriptor, vdm_wgrad_plan_info) of the launch the case makes: host only."""
    from vdm4cdm_amd import _lib
    conv = conv or conv_of(c)
    d = conv.desc(c.n, *c.grid, c.dtype)
    info = _lib.WgradPlanInfo()
    st = _lib.lib().vdm_conv_wgrad_plan(d, int(c.bias), int(c.acc), ctypes.byref(info))
    assert st == 0, _lib.lib().vdm_last_error()
    return d, info


def assert_plan(c, info):
    """The case reaches the kernel it names, with the plan fields it is there for."""
    from vdm4cdm_amd import _lib
    names = {getattr(_lib, "WGRAD_" + k): k for k in ("THIN_IN", "THIN_OUT", "ROWS", "ROWS_ROLL", "TAPSPLIT", "CLASS")}
    assert names[info.kernel] == c.kernel, f"{c.name}: the plan runs {names[info.kernel]}, the case is there for {c.kernel}"
    for k, v in c.fields.items():
        assert getattr(info, k) == v, f"{c.name}: plan {k} = {getattr(info, k)}, expected {v}"


def depths(c, info, fp32_exact):
    """(L of dw, L of dbias) of the case's launch from its plan (_wgrad_ref.py)."""
    bf16 = c.dtype == BF
    if c.kernel in ("THIN_IN", "THIN_OUT"):
        return R.depth_thin(c.n, c.grid, info.P)
    if c.kernel in ("ROWS", "ROWS_ROLL"):
        return R.depth_rows(c.kernel == "ROWS_ROLL", c.n, c.grid, info.tz, info.ty, info.tiles, info.P)
    return R.depth_tapsplit(bf16, fp32_exact, c.ks, c.kernel == "CLASS", info.tz, info.ty, info.tiles, info.P)


def real_operands(c, seed):
    """check B: randn rounded to the storage type; the conv's input offset by 0.3 so that the sums do not centre on zero."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(ishape(c) + (c.cin,), generator=g) + 0.3).to(c.dtype).float()
    dout = torch.randn((c.n,) + tuple(c.grid) + (c.cout,), generator=g).to(c.dtype).float()
    return x, dout
