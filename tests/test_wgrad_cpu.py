"""CPU side of the weight-gradient kernel checks (tests/test_wgrad_kernels_gpu.py):
  * ref_wgrad (tests/_wgrad_ref.py: plain shifted matrix products) IS the weight gradient of F.conv3d: bit-equal to float64 autograd on
    integer operands (both sums are then exact, so any difference is an indexing difference) and to 1e-13 on random reals, in every
    mode - zeros, circular, stride 2, up-sampling, ksize 1, circular grids smaller than the halo;
  * every case of the table (tests/_wgrad_cases.py) reaches the kernel it names, with the plan fields it is there for
    (vdm_conv_wgrad_plan is host only);
  * the derived bound of check B is measured against the reference, never a kernel: a plain torch-fp32 evaluation of the same sum
    (F.conv3d autograd and ref_wgrad in float32) lies inside it, and two emulated faults lie outside - the partial sum over half of
    the voxels rounded to bf16 once (a slab, an LDS fold or an accumulator kept in bf16), and for fp32 storage one operand rounded to
    bf16 (both cross terms of the split product dropped)."""
import pytest
import torch
import torch.nn.functional as F

import _wgrad_cases as W
import _wgrad_ref as R
from _exact import assert_same_bits, ints, ints_biased


def autograd_wgrad(x, dout, ks, stride, ups, circular, dtype=torch.float64):
    """The same gradient by autograd of F.conv3d, in the [ks^3, cout, cin] layout."""
    xc = x.to(dtype).permute(0, 4, 1, 2, 3)
    if ups:
        xc = F.interpolate(xc, scale_factor=2, mode="nearest")
    cout, cin, pad = dout.shape[-1], x.shape[-1], ks // 2
    w = torch.zeros(cout, cin, ks, ks, ks, dtype=dtype, requires_grad=True)
    if pad and circular:
        y = F.conv3d(F.pad(xc, (pad,) * 6, mode="circular"), w, stride=stride)
    else:
        y = F.conv3d(xc, w, stride=stride, padding=pad)
    y.backward(dout.to(dtype).permute(0, 4, 1, 2, 3))
    return w.grad.permute(2, 3, 4, 0, 1).reshape(ks ** 3, cout, cin)


# name, N, output grid, cin, cout, ks, stride, ups, circular
REF_MODES = [
    ("zeros", 2, (3, 5, 7), 3, 5, 3, 1, 0, False),
    ("circular", 2, (3, 5, 7), 3, 5, 3, 1, 0, True),
    ("circular_1x1x1", 1, (1, 1, 1), 4, 3, 3, 1, 0, True),
    ("circular_2x4x6", 1, (2, 4, 6), 4, 3, 3, 1, 0, True),
    ("stride2", 2, (2, 3, 5), 3, 4, 3, 2, 0, False),
    ("stride2_circular", 1, (1, 1, 2), 3, 4, 3, 2, 0, True),
    ("ups", 1, (4, 6, 10), 3, 4, 3, 1, 1, False),
    ("ups_circular", 2, (2, 2, 2), 3, 4, 3, 1, 1, True),
    ("ksize1", 2, (3, 5, 7), 5, 3, 1, 1, 0, False),
]


@pytest.mark.parametrize("mode", REF_MODES, ids=[m[0] for m in REF_MODES])
def test_ref_wgrad_is_autograd_of_conv3d(mode):
    name, n, grid, cin, cout, ks, stride, ups, circ = mode
    ish = R.input_shape(n, grid, stride, ups)
    nt = n * grid[0] * grid[1] * grid[2]
    for mk in (ints, ints_biased):
        x, dout = mk(ish + (cin,), 1, nt), mk((n,) + grid + (cout,), 2, nt)
        dw, abs_sum = R.ref_wgrad(x, dout, ks, stride, ups, circ)
        assert_same_bits(dw, autograd_wgrad(x, dout, ks, stride, ups, circ), f"{name}: ref_wgrad vs float64 autograd")
        assert_same_bits(abs_sum, autograd_wgrad(x.abs(), dout.abs(), ks, stride, ups, circ), f"{name}: abs_sum")
    g = torch.Generator().manual_seed(3)
    x, dout = torch.randn(ish + (cin,), generator=g, dtype=torch.float64), torch.randn((n,) + grid + (cout,), generator=g, dtype=torch.float64)
    dw, abs_sum = R.ref_wgrad(x, dout, ks, stride, ups, circ)
    assert ((dw - autograd_wgrad(x, dout, ks, stride, ups, circ)).abs() <= 1e-13 * abs_sum + 1e-300).all()


@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_case_reaches_its_kernel(case):
    d, info = W.plan_of(case)
    W.assert_plan(case, info)
    from vdm4cdm_amd import _lib
    assert info.workspace_bytes > 0 and _lib.lib().vdm_conv_wgrad_workspace_bytes(d) >= info.workspace_bytes
    L, Lb = W.depths(case, info, False)
    assert 32 < L < 400 and 32 < Lb < 400          # a chain this short keeps the bound below the emulated faults (below)


def test_case_table_covers_the_plan():
    kernels = {c.kernel for c in W.CASES}
    assert kernels == {"THIN_IN", "THIN_OUT", "ROWS", "ROWS_ROLL", "TAPSPLIT", "CLASS"}
    for k in kernels - {"THIN_IN", "THIN_OUT"}:
        assert any(c.acc for c in W.CASES if c.kernel == k), f"no accumulate case for {k}"
    assert not any(c.acc for c in W.CASES if c.kernel in ("THIN_IN", "THIN_OUT"))
    thin_in = [c for c in W.CASES if c.kernel == "THIN_IN"]
    thin_out = [c for c in W.CASES if c.kernel == "THIN_OUT"]
    grids = {(n, g, circ) for n, g, circ in W.THIN_GRIDS.values()}
    assert {c.cin for c in thin_in} == {1, 2} and {c.cout for c in thin_in} == {16, 32, 64} and {(c.n, c.grid, c.circ) for c in thin_in} == grids
    assert {c.cin for c in thin_out} == {16, 32, 64} and {(c.n, c.grid, c.circ) for c in thin_out} == grids
    assert all(W.BY_NAME[b].acc is False for b in W.B_CASES)
    assert {W.BY_NAME[b].kernel for b in W.B_CASES} == kernels


# ---------------------------------------------------------------------------------------------------------------- check B, CPU half
def _b_setups():
    """(id, case, fp32 build): bf16 storage has one build, fp32 storage the split default and the exact one."""
    out = []
    for name in W.B_CASES:
        c = W.BY_NAME[name]
        out += [(name, c, False)] if c.dtype == W.BF else [(name + "_split", c, False), (name + "_exact", c, True)]
    return out


B_SETUPS = _b_setups()


@pytest.mark.parametrize("setup", B_SETUPS, ids=[s[0] for s in B_SETUPS])
def test_bound_admits_fp32_and_rejects_faults(setup):
    name, c, fp32_exact = setup
    bf16 = c.dtype == W.BF
    L, Lb = W.depths(c, W.plan_of(c)[1], fp32_exact)
    eps = R.eps_op(bf16, fp32_exact)
    x, dout = W.real_operands(c, 7)
    ref, abs_sum = R.ref_wgrad(x, dout, c.ks, c.stride, c.ups, c.circ)
    bnd = R.bound(abs_sum, L, eps)
    u = R.U32 * abs_sum
    # 1. inside: the same sum in torch fp32, two ways
    for what, got in (("conv3d autograd fp32", autograd_wgrad(x, dout, c.ks, c.stride, c.ups, c.circ, torch.float32)),
                      ("ref_wgrad fp32", R.ref_wgrad(x, dout, c.ks, c.stride, c.ups, c.circ, torch.float32)[0])):
        err = (got.double() - ref).abs()
        print(f"{name}: {what}: max err {(err / u).max().item():.2f} u abs_sum, bound {(bnd / u).min().item():.0f} u abs_sum")
        assert (err <= bnd).all(), f"{name}: {what} outside the derived bound: {(err / bnd).max().item():.3f}"
    # 2. outside: half of the voxels' partial sum rounded to bf16 once
    half = dout.clone()
    half.view(-1, c.cout)[half.view(-1, c.cout).shape[0] // 2:] = 0
    part = R.ref_wgrad(x, half, c.ks, c.stride, c.ups, c.circ)[0]
    err = (part.float().bfloat16().double() - part).abs()
    print(f"{name}: bf16 slab fault: max err {(err / u).max().item():.0f} u abs_sum")
    assert (err > bnd).any(), f"{name}: the bound (L = {L}) does not notice a partial sum kept in bf16: {(err / bnd).max().item():.3f}"
    # dbias: the same bound with abs_sum = sum |dout|
    if c.bias:
        g = dout.reshape(-1, c.cout).double()
        bb = R.bound(g.abs().sum(0), Lb, eps)
        assert ((g.float().sum(0).double() - g.sum(0)).abs() <= bb).all()
        hp = g[:g.shape[0] // 2].sum(0)
        assert ((hp.float().bfloat16().double() - hp).abs() > bb).any(), f"{name}: the dbias bound (L = {Lb}) does not notice a bf16 partial"
    # 3. outside, fp32 storage: one operand rounded to bf16
    if not bf16:
        got = R.ref_wgrad(x.bfloat16().float(), dout, c.ks, c.stride, c.ups, c.circ)[0]
        err = (got - ref).abs()
        print(f"{name}: bf16 operand fault: max err {(err / u).max().item():.0f} u abs_sum")
        assert (err > bnd).any(), f"{name}: the bound does not notice an operand rounded to bf16: {(err / bnd).max().item():.3f}"
