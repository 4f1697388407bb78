"""CPU reference and error bounds of the weight-gradient kernel checks (tests/test_wgrad_cpu.py, tests/test_wgrad_kernels_gpu.py).

ref_wgrad is the weight gradient as 27 (or 1) plain shifted matrix products in float64 - no F.conv3d, no autograd, nothing shared with
ref_conv of test_kernels_gpu.py.  The bound of check B is
    |dw - ref| <= (eps_op + L * 2^-24) * abs_sum + 2^-126,       abs_sum[t] = |dout|^T |x shifted by tap t|
with eps_op the relative error of one PRODUCT and L the number of fp32 additions one product passes through on its way into dw, both
read off the kernels (csrc/conv_wgrad.hip, csrc/wgrad_thin.hip) and computed from the plan of the launch - never
from a kernel's results."""
import torch

U32 = 2.0 ** -24                      # unit roundoff of fp32
FLOOR = 2.0 ** -126

# eps_op.  bf16 storage: a product of two bf16 values has 16 significant bits - exact in fp32.  fp32 storage, default build
# (csrc/common.h split_frag): an operand is hi + lo + r with |r| <= 2^-18 |x| (two bf16 roundings of 2^-9 each), the product is formed as
# hi_a lo_b + lo_a hi_b + hi_a hi_b: dropped are a r_b, b r_a (2^-18 each) and lo_a lo_b (2^-18: |lo| <= 2^-9 |x|), second-order terms
# below 0.01 * 2^-18.  Exact build (VDM4CDM_FP32_EXACT=1, v_mfma_f32_16x16x4_f32: a chain of fmas): the one rounding of the product's fma.
EPS_SPLIT = 3.01 * 2.0 ** -18
EPS_EXACT = 2.0 ** -24


def eps_op(bf16, fp32_exact):
    return 0.0 if bf16 else (EPS_EXACT if fp32_exact else EPS_SPLIT)


def input_shape(n, grid, stride, ups):
    """Spatial shape of the conv's input for an OUTPUT grid (D, H, W)."""
    D, H, W = grid
    if stride == 2:
        return (n, 2 * D, 2 * H, 2 * W)
    if ups:
        assert D % 2 == 0 and H % 2 == 0 and W % 2 == 0
        return (n, D // 2, H // 2, W // 2)
    return (n, D, H, W)


def _padded(x, pad, circular):
    """x [N, D, H, W, C] with `pad` voxels of explicit zero or circular padding on every side of the three spatial axes."""
    if pad == 0:
        return x
    n, d, h, w, c = x.shape
    if circular:
        for axis, size in ((1, d), (2, h), (3, w)):
            idx = torch.arange(-pad, size + pad) % size          # a true modulo: a grid smaller than the halo wraps more than once
            x = x.index_select(axis, idx)
        return x
    out = x.new_zeros((n, d + 2 * pad, h + 2 * pad, w + 2 * pad, c))
    out[:, pad:pad + d, pad:pad + h, pad:pad + w] = x
    return out


def ref_wgrad(x, dout, ks, stride, ups, circular, dtype=torch.float64):
    """x [N, Di, Hi, Wi, cin], dout [N, D, H, W, cout] -> (dw, abs_sum), both [ks^3, cout, cin] in `dtype`:
    dw[t][co][ci] = sum_{n, v} dout[n][v][co] * xpad[n][stride * v + (dz, dy, dx)][ci],  t = (dz * 3 + dy) * 3 + dx,
    xpad = the (nearest x2 up-sampled, if `ups`) input with ks // 2 voxels of zero / circular padding."""
    x, dout = x.to(dtype), dout.to(dtype)
    if ups:
        for axis in (1, 2, 3):
            x = x.repeat_interleave(2, dim=axis)
    n, D, H, W, cout = dout.shape
    cin = x.shape[-1]
    assert tuple(x.shape[:4]) == (n, stride * D, stride * H, stride * W), f"input {tuple(x.shape)} does not fit dout {tuple(dout.shape)}"
    xp = _padded(x, ks // 2, circular)
    g = dout.reshape(-1, cout)
    ga = g.abs()
    dw = torch.empty((ks ** 3, cout, cin), dtype=dtype)
    abs_sum = torch.empty_like(dw)
    for dz in range(ks):
        for dy in range(ks):
            for dx in range(ks):
                t = (dz * ks + dy) * ks + dx
                xs = xp[:, dz:dz + stride * D:stride, dy:dy + stride * H:stride, dx:dx + stride * W:stride].reshape(-1, cin)
                dw[t] = g.t() @ xs
                abs_sum[t] = ga.t() @ xs.abs()
    return dw, abs_sum


def bound(abs_sum, L, eps):
    return (eps + L * U32) * abs_sum + FLOOR


# ---------------------------------------------------------------------------------------------------------------------------------
# L: the fp32 additions one product passes through.  Every function returns (L of dw, L of dbias).
# ---------------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def mfma_shape(bf16, fp32_exact):
    """(products summed inside one MFMA, roundings of the accumulator register per k-step).  bf16: one v_mfma_f32_16x16x32_bf16, the sum
    of its 32 exact products is added to the accumulator.  fp32 default: three v_mfma_f32_16x16x16_bf16 (mma16_ss), 16 products each.
    fp32 exact: four v_mfma_f32_16x16x4_f32, each a CHAIN of 4 fmas on the accumulator - 16 roundings of the running sum per k-step."""
    if bf16:
        return 32, 1
    return (4, 16) if fp32_exact else (16, 3)


def _slab_reduce(nslabs):
    """wgrad_reduce_direct_kernel (<= 32 slabs: one thread adds them in turn) or wgrad_reduce_kernel (four groups add every fourth
    slab in turn, then the four group sums are added in turn).  The larger of the two where either may run (VDM4CDM_EXPERIMENT=grouped_reduce)."""
    grouped = cdiv(nslabs, 4) + 4
    return grouped if nslabs > 32 else max(nslabs, grouped)


def _bias_reduce(nslabs):
    """wgrad_bias_reduce_kernel: 16 groups add every 16th partial in turn, then the 16 group sums are added in turn."""
    return cdiv(nslabs, 16) + 16


def depth_tapsplit(bf16, fp32_exact, ks, cls, tz, ty, tiles, P):
    """conv_wgrad_kernel (VDM_WGRAD_TAPSPLIT, VDM_WGRAD_CLASS).  A wave owns its taps and walks every k-step (bf16: two rows of 16 voxels,
    fp32: one row) of every tile of its workgroup, ceil(tiles / P) of them; ksize 1: the four waves split the k-steps and write a slab
    each.  No fold across waves.  CLASS: a master tap is the sum of one merged tap of each of the 8 parity classes
    (wgrad_cls_reduce_kernel: four groups add every fourth of the P slabs of the 8 sources in turn, then the four group sums).
    dbias: a lane adds one value per row it owns (rows / 4 per tile), 64 lane sums are folded in turn (4 waves x 16 voxels), then the
    bias reduce over P (CLASS: 8 P) partials."""
    inner, per_kstep = mfma_shape(bf16, fp32_exact)
    rows = tz * ty
    ksteps = rows // (2 if bf16 else 1)
    if ks == 1:
        ksteps = cdiv(ksteps, 4)
    per_wg_tiles = cdiv(tiles, P)
    reduce = 8 * cdiv(P, 4) + 4 if cls else _slab_reduce(P * (4 if ks == 1 else 1))
    L = inner + per_kstep * ksteps * per_wg_tiles + reduce
    Lb = cdiv(rows, 4) * per_wg_tiles + 64 + _bias_reduce(P * (8 if cls else 1))
    return L, Lb


def depth_rows(roll, n, grid, tz, ty, tiles, P):
    """conv_wgrad_rows_kernel (VDM_WGRAD_ROWS, VDM_WGRAD_ROWS_ROLL; bf16).  A wave owns one 16 x 16 tile of all 27 taps; a step (one
    tz x ty x 16 tile) adds tz * ty / 2 MFMAs into each tap's register (wgrad_rows_step: per output slab ty / 2 k-steps for dy = 0 and
    dy = 2, ty / 2 - 1 plus the wrap k-step for dy = 1).  ROWS: ceil(tiles / P) steps per workgroup.  ROLL: `tiles` counts column
    segments, ceil(tiles / P) of them per workgroup, zsteps steps each.  dbias: the same MFMAs against a fragment of ones."""
    D, H, W = grid
    steps = cdiv(tiles, P)
    if roll:
        ncols = n * cdiv(H, ty) * cdiv(W, 16)
        assert tiles % ncols == 0
        steps *= cdiv(cdiv(D, tz), tiles // ncols)                # zsteps = ceil(z tiles / segments per column)
    mfmas = (tz * ty // 2) * steps
    return 32 + mfmas + _slab_reduce(P), 32 + mfmas + _bias_reduce(P)


def depth_thin(n, grid, P):
    """wgrad_thin_kernel (VDM_WGRAD_THIN_IN / _OUT; bf16).  One MFMA per chunk of 32 x-consecutive voxels; the 4 P waves take every
    (4 P)th chunk; the four waves of a workgroup are added in turn through LDS; wgrad_thin_reduce_kernel: 16 groups add every 16th
    slab in turn, then the 16 group sums in turn.  dbias is column 72 of the same product."""
    D, H, W = grid
    chunks = n * D * H * cdiv(W, 32)
    L = 32 + cdiv(chunks, 4 * P) + 4 + cdiv(P, 16) + 16
    return L, L
