"""CPU reference and error bounds of the forward / input-gradient conv kernel checks (tests/test_conv_cpu.py,
tests/test_conv_kernels_gpu.py).

ref_fwd is the convolution as 27 (or 1) plain shifted matrix products in float64, ref_dgrad the explicit transpose of that sum (every
dout x W product scattered to the input voxel it came from) - no F.conv3d, no autograd, nothing shared with ref_conv of
test_kernels_gpu.py.  Both return (result, abs_sum), abs_sum being the same expression over absolute values.  The bound of check B is
    |out - ref| <= (eps_op + L * 2^-24) * abs_sum + eps_merge * abs_conv + store(ref) + 2^-126
with eps_op the relative error of one PRODUCT (_wgrad_ref.eps_op), L the number of fp32 additions one product passes through on its way
into the output (depth() below), eps_merge the rounding of a merged class weight (class kernels of the up-sampling conv only; abs_conv
is abs_sum without the epilogue terms) and store() the one rounding to the output type.  All of it is read off the kernels
(csrc/conv_fwd.hip, csrc/conv_cls.hip, csrc/conv_common.h, the packer in csrc/conv_api.hip) and computed from the plan of the launch -
never from a kernel's results."""
import torch

from _gn_bounds import UB, store_err
from _wgrad_ref import FLOOR, U32, _padded, cdiv, eps_op, input_shape, mfma_shape      # noqa: F401  (re-exported to the tests)


def _taps(ks):
    return [(dz, dy, dx) for dz in range(ks) for dy in range(ks) for dx in range(ks)]


def add_epilogue(out, abs_sum, bias=None, nbias=None, res=None):
    """The header's epilogue: out = conv + bias[c] + nbias[n][c] + residual, in the dtype of `out`; abs_sum grows by the absolute values."""
    for t, shape in ((bias, (1, 1, 1, 1, -1)), (nbias, (out.shape[0], 1, 1, 1, -1)), (res, out.shape)):
        if t is not None:
            t = t.to(out.dtype).reshape(shape)
            out = out + t
            abs_sum = None if abs_sum is None else abs_sum + t.abs()
    return out, abs_sum


def ref_fwd(x, w, ks, stride, ups, circular, bias=None, nbias=None, res=None, dtype=torch.float64, want_abs=True):
    """x [N, Di, Hi, Wi, cin], w [ks^3, cout, cin] (tap t = (dz * 3 + dy) * 3 + dx) -> (out, abs_sum), both [N, D, H, W, cout] in `dtype`:
    out[n][v][co] = sum_{t, ci} xpad[n][stride * v + (dz, dy, dx)][ci] * w[t][co][ci] + bias[co] + nbias[n][co] + res[n][v][co],
    xpad = the (nearest x2 up-sampled, if `ups`) input with ks // 2 voxels of zero / circular padding."""
    x, w = x.to(dtype), w.to(dtype)
    if ups:
        for axis in (1, 2, 3):
            x = x.repeat_interleave(2, dim=axis)
    n, Di, Hi, Wi, cin = x.shape
    assert Di % stride == 0 and Hi % stride == 0 and Wi % stride == 0
    D, H, W = Di // stride, Hi // stride, Wi // stride
    cout = w.shape[1]
    xp = _padded(x, ks // 2, circular)
    out = torch.zeros((n * D * H * W, cout), dtype=dtype)
    abs_sum = torch.zeros_like(out) if want_abs else None
    for t, (dz, dy, dx) in enumerate(_taps(ks)):
        xs = xp[:, dz:dz + stride * D:stride, dy:dy + stride * H:stride, dx:dx + stride * W:stride].reshape(-1, cin)
        out += xs @ w[t].t()
        if want_abs:
            abs_sum += xs.abs() @ w[t].abs().t()
    shape = (n, D, H, W, cout)
    return add_epilogue(out.view(shape), abs_sum.view(shape) if want_abs else None, bias, nbias, res)


def ref_dgrad(dout, w, ks, stride, ups, circular, res=None, dtype=torch.float64, want_abs=True):
    """dout [N, D, H, W, cout] -> (dx, abs_sum), both [N, Di, Hi, Wi, cin]: the transpose of ref_fwd's sum.  Every product
    dout[n][v][co] * w[t][co][ci] is added to the voxel stride * v + (dz, dy, dx) of the PADDED (up-sampled) input grid; a padding voxel
    then hands its sum to the voxel it wraps onto (circular: true modulo) or drops it (zeros), and the 2x2x2 fine voxels that an
    up-sampling conv read from one source voxel are summed.  `res` (the gradient being accumulated into) is added at the end."""
    dout, w = dout.to(dtype), w.to(dtype)
    n, D, H, W, cout = dout.shape
    cin, pad = w.shape[2], ks // 2
    fine = (stride * D, stride * H, stride * W)
    g = dout.reshape(-1, cout)
    outs = []
    for gg, ww in ((g, w), (g.abs(), w.abs())) if want_abs else ((g, w),):
        dxp = torch.zeros((n, fine[0] + 2 * pad, fine[1] + 2 * pad, fine[2] + 2 * pad, cin), dtype=dtype)
        for t, (dz, dy, dx) in enumerate(_taps(ks)):
            dxp[:, dz:dz + stride * D:stride, dy:dy + stride * H:stride, dx:dx + stride * W:stride] += (gg @ ww[t]).view(n, D, H, W, cin)
        for axis, size in ((1, fine[0]), (2, fine[1]), (3, fine[2])):
            if pad == 0:
                continue
            if circular:
                idx = torch.arange(-pad, size + pad) % size
                shape = list(dxp.shape)
                shape[axis] = size
                dxp = torch.zeros(shape, dtype=dtype).index_add_(axis, idx, dxp)
            else:
                dxp = dxp.narrow(axis, pad, size)
        if ups:
            dxp = dxp.reshape(n, fine[0] // 2, 2, fine[1] // 2, 2, fine[2] // 2, 2, cin).sum(dim=(2, 4, 6))
        outs.append(dxp.contiguous())
    return add_epilogue(outs[0], outs[1] if want_abs else None, None, None, res)


# ---------------------------------------------------------------------------------------------------------------------------------
# The parity classes of the class kernels (csrc/conv_common.h cls_dim_entries): per dimension and parity p the entries
# (coarse offset o, master taps merged into the entry).  Used by the CPU emulation of the kernels' summation order.
# ---------------------------------------------------------------------------------------------------------------------------------
def cls_dim_entries(kind, p):
    if kind == "S2_DGRAD":
        return [(0, (1,))] if p == 0 else [(1, (0,)), (0, (2,))]
    return [(-1, (0,)), (0, (1, 2))] if p == 0 else [(0, (0, 1)), (1, (2,))]


def cls_entries(kind, cl):
    """[(oz, oy, ox), [master taps]] of class cl = (pz * 2 + py) * 2 + px, in the kernel's entry order."""
    p = ((cl >> 2) & 1, (cl >> 1) & 1, cl & 1)
    ez, ey, ex = (cls_dim_entries(kind, q) for q in p)
    return [((oz, oy, ox), [(tz * 3 + ty) * 3 + tx for tz in sz for ty in sy for tx in sx])
            for oz, sz in ez for oy, sy in ey for ox, sx in ex]


# ---------------------------------------------------------------------------------------------------------------------------------
# L: the fp32 additions one product passes through, and the bound
# ---------------------------------------------------------------------------------------------------------------------------------
def depth(family, cls_kind, bf16, fp32_exact, ks, nkb, epilogue_terms):
    """One MFMA adds the sum of its `inner` products to the accumulator register (mfma_shape: bf16 32 products and one rounding of the
    register per K-step; fp32 storage three MFMAs of 16, or in the exact build a chain of 16 fmas).  The register then takes every
    later MFMA of its chain:
      GENERIC, SPLIT, rolling z (conv_fwd_kernel, conv_roll_kernel): taps x K-blocks K-steps, K-blocks outermost;
      KSPLIT (conv_ksplit_kernel): a wave takes every fourth K-block - taps x ceil(nkb / 4) K-steps - and the four waves' registers are
          added as (p0 + p1) + (p2 + p3): 2 more;
      KPACK (conv_kpack_kernel): 7 tap groups;
      CLASS (conv_cls_kernel): at most 8 entries per class and K-block; the up-sampling conv's input gradient keeps accumulating over
          its 8 classes: 64 entries per K-block.
    Epilogue (conv_epilogue, cls_epilogue): badd = bias + nbias is formed (1), added (1), then the residual (1) - `epilogue_terms` of
    them for the terms the call passes; the rounding of the store is store() of the bound."""
    inner, per_kstep = mfma_shape(bf16, fp32_exact)
    if family == "KPACK":
        chain = 7
    elif family == "KSPLIT":
        chain = ks ** 3 * cdiv(nkb, 4) + 2
    elif family == "CLASS":
        chain = (64 if cls_kind == "UP_DGRAD" else 8) * nkb
    else:
        chain = ks ** 3 * nkb
    return inner + per_kstep * chain + epilogue_terms


def eps_merge(family, cls_kind, bf16):
    """Class kernels of the up-sampling conv: pack_value adds the <= 8 master taps of an entry in fp32 (7 additions) and stores the sum in
    the storage type - bf16: one more rounding, 2^-8 relative (8 significant bits); fp32: the split of the stored value is eps_op's.  Relative to
    sum |master taps| |x| = abs_conv.  The stride-2 input gradient has one master tap per entry: nothing is merged."""
    if family != "CLASS" or cls_kind == "S2_DGRAD":
        return 0.0
    return 7 * U32 + (UB if bf16 else 0.0)


def bound(ref, abs_sum, abs_conv, L, eps, epsm, out_bf16):
    return store_err(ref, (eps + L * U32) * abs_sum + epsm * abs_conv, out_bf16) + FLOOR
