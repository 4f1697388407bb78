"""Kernel-level parity tests of the six weight-gradient kernels, the VDM_WGRAD_* kernels that plan_wgrad picks between
(csrc/conv_common.h; csrc/conv_wgrad.hip, csrc/wgrad_thin.hip), each through vdm_conv_wgrad with a workspace of its own.  The cases are
in tests/_wgrad_cases.py; tests/test_wgrad_cpu.py confirms their plans and the bound of check B without a device.

Two kinds of check, because they catch different faults:
  A. exact integers, no tolerance.  Operands are small integers in the storage type (exact in bf16), so every product and every partial
     sum is an integer below 2^24 and fp32 addition is exact in any order: dw and dbias must have the BITS of the float64 sum of
     ref_wgrad (tests/_wgrad_ref.py) - a dropped, duplicated or mis-wrapped voxel, a missing boundary row of a ragged tile, a padded dout
     voxel read as circular all show, and the mismatch pattern (taps, tile face, sample) names the fault.  Every case runs with
     integers in {-2..2} and again in {0..3}: the biased sums grow to ~2.25 x voxels, which an accumulator, LDS fold or slab held in
     less than fp32 cannot carry (signed data hides that).  The workspace holds exactly the plan's bytes and is 0xFF (every float a
     NaN) before every call, so a slab slot that is read but never written poisons the result; dw / dbias lie inside sentinel buffers
     and start as NaN (accumulate: as integers in [-8, 8], and must end as start + reference).  A second call gives the same bits.
  B. random reals against ref_wgrad in float64, operands rounded to the storage type first, per element
         |dw - ref| <= (eps_op + L * 2^-24) * abs_sum + 2^-126
     with eps_op the error of one product (0 for bf16 storage; 3.01 * 2^-18 for fp32 storage on the bf16 pipe, 2^-24 in the
     VDM4CDM_FP32_EXACT build) and L the fp32 additions one product passes through, derived per kernel from the code and computed
     from the plan of the launch (_wgrad_ref.py depth_*), never fitted.  dbias: the same with abs_sum = sum |dout|.

B, measured max over the elements of err / bound on an MI355X, default build (kernel, L of dw / dbias: dw | dbias):
  roll_half_ztile          ROWS_ROLL   56 /  65   0.013 | 0.001
  roll_grouped_reduce      ROWS_ROLL   76 /  70   0.001 | 0.000
  rows_one_ztile           ROWS        45 /  57   0.027 | 0.000
  rows_256_scattered       ROWS        64 /  73   0.009 | 0.001
  tapsplit_16_32           TAPSPLIT    52 /  85   0.013 | 0.001
  f32_20_24_circ           TAPSPLIT    72 /  85   0.085 | 0.001      (fp32 storage: eps_op = 3.01 * 2^-18 = 193 * 2^-24 on top of L)
  s2_32_64_bf16            TAPSPLIT    40 /  82   0.026 | 0.001
  s2_32_64_f32             TAPSPLIT    34 /  82   0.222 | 0.004
  k1_64_32_bf16            TAPSPLIT    56 /   -   0.005 | -
  ups_64_32_bf16           CLASS       52 /  85   0.009 | 0.001
  thin_in_1_16_5x7x33      THIN_IN     55 /  55   0.012 | 0.000
  thin_in_2_32_16x33x40    THIN_IN     86 /  86   0.001 | 0.000
  thin_out_32_4x4x70_circ  THIN_OUT    55 /   -   0.004 | -
  (the bound is a worst case over the signs of L roundings; random roundings err like sqrt(L), and the large grids average over
  10^4 - 10^5 voxels.  The emulated faults of tests/test_wgrad_cpu.py exceed the same bounds 7 to 480 times.)
"""
import pytest
import torch

import _wgrad_cases as W
import _wgrad_ref as R
from _exact import assert_same_bits, in_sentinel, ints, ints_biased

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                          # bytes behind the workspace (0xA5): nothing may be written there
DISTS = {"signed": ints, "biased": ints_biased}


def _mods():
    from vdm4cdm_amd import _lib
    from vdm4cdm_amd import hip_ops
    return _lib, hip_ops


def _padded_dev(t, dtype, cpad):
    """[..., c] fp32 on the CPU -> [..., cpad] in the storage type on the device, padding channels zero (as the ABI says)."""
    out = torch.zeros(t.shape[:-1] + (cpad,), dtype=dtype, device=DEV)
    out[..., :t.shape[-1]] = t.to(dtype).to(DEV)
    return out


def _start(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g, dtype=torch.int8).float()


class Launch:
    """One vdm_conv_wgrad launch of a case the way a caller with its own buffers makes it: workspace of exactly the plan's bytes
    (poisoned), dw / dbias as views inside sentinel buffers."""

    def __init__(self, c, x, dout):
        _lib, ops = _mods()
        self.c, self.L = c, _lib.lib()
        self.conv = W.conv_of(c)
        self.d, self.info = W.plan_of(c, self.conv)
        W.assert_plan(c, self.info)                                     # the case is wrong if the plan says otherwise
        self.need = self.info.workspace_bytes
        self.xd = _padded_dev(x, c.dtype, ops.cpad(c.cin, c.dtype))
        self.dd = _padded_dev(dout, c.dtype, ops.cpad(c.cout, c.dtype))
        self.ws = torch.empty(self.need + GUARD, dtype=torch.uint8, device=DEV)
        self.ws[self.need:] = 0xA5
        taps = c.ks ** 3
        self.dw_buf, self.dw, self.dw_ok = in_sentinel(taps * c.cout * c.cin, (taps, c.cout, c.cin))
        self.db_buf, self.db, self.db_ok = in_sentinel(c.cout, (c.cout,)) if c.bias else (None, None, lambda: True)

    def run(self, dw0=None, db0=None):
        """dw0 / db0: the start values of an accumulate call (CPU); otherwise the outputs start as NaN.  Returns (dw, dbias) on the CPU."""
        c = self.c
        self.ws[:self.need] = 0xFF
        for t, t0 in ((self.dw, dw0), (self.db, db0)):
            if t is not None:
                t.copy_(t0) if c.acc else t.fill_(float("nan"))
        st = self.L.vdm_conv_wgrad(self.d, self.xd.data_ptr(), self.dd.data_ptr(), self.dw.data_ptr(),
                                   None if self.db is None else self.db.data_ptr(), int(c.acc), self.ws.data_ptr(), self.need,
                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert st == 0, self.L.vdm_last_error()
        assert bool((self.ws[self.need:] == 0xA5).all()), f"{c.name}: bytes behind the workspace were written"
        assert self.dw_ok() and self.db_ok(), f"{c.name}: bytes around dw / dbias were written"
        dw, db = self.dw.cpu().clone(), (None if self.db is None else self.db.cpu().clone())
        assert not torch.isnan(dw).any() and (db is None or not torch.isnan(db).any()), f"{c.name}: NaN in the result (a slab slot read but never written)"
        return dw, db


# =============================================================================================== A: exact integers
@pytest.mark.parametrize("dist", list(DISTS), ids=list(DISTS))
@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_wgrad_exact_integers(case, dist):
    c, mk = case, DISTS[dist]
    nt = W.terms(c)
    x, dout = mk(W.ishape(c) + (c.cin,), 11, nt), mk((c.n,) + tuple(c.grid) + (c.cout,), 12, nt)
    ref, _ = R.ref_wgrad(x, dout, c.ks, c.stride, c.ups, c.circ)
    bref = dout.double().reshape(-1, c.cout).sum(0)
    dw0 = _start(ref.shape, 13) if c.acc else None
    db0 = _start(bref.shape, 14) if c.acc else None
    assert ref.abs().max().item() + 8 < 2 ** 24
    if c.acc:
        ref, bref = ref + dw0.double(), bref + db0.double()
    run = Launch(c, x, dout)
    dw, db = run.run(dw0, db0)
    assert_same_bits(dw, ref, f"{c.name}/{dist}: dw [tap, cout, cin]")
    if c.bias:
        assert_same_bits(db, bref, f"{c.name}/{dist}: dbias")
    dw2, db2 = run.run(dw0, db0)
    assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2)), f"{c.name}/{dist}: a second call gives other bits"


def test_wgrad_k1_refuses_a_bias_gradient():
    """ksize 1 has no fused bias gradient: VDM_ERR_UNSUPPORTED before any launch stays the contract."""
    c = W.BY_NAME["k1_64_32_bf16"]
    run = Launch(c, ints(W.ishape(c) + (c.cin,), 1, W.terms(c)), ints((c.n,) + tuple(c.grid) + (c.cout,), 2, W.terms(c)))
    run.dw.fill_(float("nan"))
    db = torch.full((c.cout,), float("nan"), device=DEV)
    st = run.L.vdm_conv_wgrad(run.d, run.xd.data_ptr(), run.dd.data_ptr(), run.dw.data_ptr(), db.data_ptr(), 0, run.ws.data_ptr(), run.need,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st != 0 and b"bias" in run.L.vdm_last_error()
    assert bool(torch.isnan(run.dw).all()) and bool(torch.isnan(db).all())


# =============================================================================================== B: random reals, derived bound
def _check_bound(name, dw, db, x, dout, ks, stride, ups, circ, L, Lb, eps):
    ref, abs_sum = R.ref_wgrad(x, dout, ks, stride, ups, circ)
    ratio = ((dw.double() - ref).abs() / R.bound(abs_sum, L, eps)).max().item()
    msg = f"B {name}: dw max err / bound = {ratio:.3f} (L = {L})"
    rb = None
    if db is not None:
        g = dout.double().reshape(-1, dout.shape[-1])
        rb = ((db.double() - g.sum(0)).abs() / R.bound(g.abs().sum(0), Lb, eps)).max().item()
        msg += f", dbias {rb:.3f} (L = {Lb})"
    print(msg)
    assert ratio <= 1.0, msg
    assert rb is None or rb <= 1.0, msg


@pytest.mark.parametrize("name", W.B_CASES)
def test_wgrad_random_reals_within_derived_bound(name):
    _lib, _ = _mods()
    c = W.BY_NAME[name]
    x, dout = W.real_operands(c, 7)
    run = Launch(c, x, dout)
    dw, db = run.run()
    L, Lb = W.depths(c, run.info, _lib.FP32_EXACT)
    _check_bound(name, dw, db, x, dout, c.ks, c.stride, c.ups, c.circ, L, Lb, R.eps_op(c.dtype == W.BF, _lib.FP32_EXACT))
