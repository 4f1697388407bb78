"""Kernel-level parity tests of csrc/attention.hip: attn_fwd_kernel, attn_bwd_kv_kernel, attn_bwd_q_kernel (through vdm_attn_fwd /
vdm_attn_bwd with buffers of the test's own, and through hip_ops.attn_bwd), attn_split_heads_kernel and attn_rowdot_kernel.  The cases
are in tests/_attention_cases.py, the references in tests/_attention_ref.py; tests/test_attention_cpu.py shows without a device that
the operands leave the bounds room and that an emulated fault of each kind fails a check A.

Two kinds of check, because they catch different faults:
  A. exact, no tolerance (bf16 outputs: the reference rounded once to bf16).
     A1 one-hot forward: k has V distinct rows of +-1, q_i = k[pi(i)], scale = 64, so P is exactly one-hot: out[i] must have the bits of
        v[pi(i)] for random real v, lse must be 64 hd.  pi(0) = V - 1 and pi(V - 1) = 0: the match arrives in the last tile for the first
        query (every earlier tile is rescaled to 0) and in the first tile for the last one.  A wrong key order between P and V^T, a
        swapped bf16 sub-tile, a missing rescale, a wrong mask or clamp, a wrong head / sample offset all show, and the mismatch pattern
        names the fault.  want_lse=False gives the same bits and leaves lse alone.
     A2 uniform forward: q = 0 and integer v, so l = V and the accumulator is the integer column sum: a key counted twice or dropped in
        the ragged tile changes l.  Bit-exact for V a power of two, otherwise within the roundings of 1 / V and of the product.
     A3 one-hot backward with an integer dsum passed in: dQ, dK, dV against int64 index arithmetic; a second call gives the same bits;
        hip_ops.attn_bwd(dsum=...) gives the same bits as the direct call.
     A4 the same data on the default path (out of A1's kind, dsum from vdm_attn_rowdot): dP = dsum exactly, so dQ = dK = 0.
     A5 attn_split_heads: every (nsub, sub), both outputs / rowmajor=False / transposed=False, bit-exact copies.
     A6 vdm_attn_rowdot on integers, and once with N V H > 4096 x 256 (the grid-stride loop).
     A7 isolation: every (sample, head) of the N = 2, H = 3 case against a launch on that slice alone, bit for bit.
     A8 containment, in A1 - A4 and B: every input (q, k, v, q^T, k^T, v^T, dO, dO^T, lse, dsum) is a 16-byte aligned view at least 256
        bytes inside a NaN-filled buffer - a clamped load that leaves the tensor and reaches an accumulator shows as NaN, and nothing
        faults - and every output (out, lse, dqkv) a view inside a sentinel buffer whose sentinels must survive; outputs start as NaN.
  B. random N(0, 1) reals, rounded to the storage type, against float64, at scale 1 / sqrt(hd) and 4 / sqrt(hd) (scores of standard
     deviation 1 and 4):
         out, bf16   per element |out - ref| <= 2^-7 (A + |ref|) + 1e-6, A = sum_j P_ij |v_jd|: twice the first-order worst case of
                     P rounded to bf16 plus one storage rounding
         out, fp32   2e-5 max |ref|
         lse         1e-4 in both dtypes (the statistics are fp32 from the same operands)
         dQ, dK, dV  each block on its own against BWD_TOL of max |ref block|

B, measured max err / bound on an MI355X, default build (the VDM4CDM_FP32_EXACT build passes with the same fp32 figures: attention uses
the exact fp32 MFMA in both).  Columns: out  lse  dQ  dK  dV at scale 1 / sqrt(hd) | the same at 4 / sqrt(hd):
  n1_h1_v4_hd16    f32   0.005  0.001  0.017  0.013  0.010 | 0.008  0.003  0.014  0.024  0.020
  n1_h1_v4_hd16    bf16  0.179  0.001  0.064  0.088  0.105 | 0.185  0.001  0.105  0.178  0.105
  n1_h2_v8_hd32    f32   0.010  0.004  0.066  0.043  0.016 | 0.013  0.019  0.081  0.138  0.023
  n1_h2_v8_hd32    bf16  0.290  0.002  0.184  0.097  0.116 | 0.317  0.007  0.173  0.235  0.161
  n1_h2_v12_hd32   f32   0.012  0.004  0.023  0.029  0.017 | 0.025  0.015  0.076  0.082  0.046
  n1_h2_v12_hd32   bf16  0.248  0.003  0.095  0.092  0.109 | 0.257  0.007  0.140  0.203  0.107
  n2_h1_v20_hd16   f32   0.013  0.003  0.012  0.011  0.024 | 0.013  0.008  0.082  0.104  0.022
  n2_h1_v20_hd16   bf16  0.209  0.003  0.097  0.108  0.130 | 0.254  0.007  0.250  0.386  0.102
  n1_h2_v24_hd16   f32   0.009  0.004  0.034  0.017  0.029 | 0.015  0.016  0.037  0.066  0.035
  n1_h2_v24_hd16   bf16  0.201  0.004  0.101  0.101  0.137 | 0.294  0.010  0.162  0.266  0.075
  n2_h1_v28_hd64   f32   0.025  0.006  0.040  0.032  0.032 | 0.046  0.039  0.045  0.055  0.058
  n2_h1_v28_hd64   bf16  0.238  0.005  0.082  0.071  0.108 | 0.278  0.013  0.104  0.092  0.088
  n1_h3_v36_hd128  f32   0.047  0.007  0.044  0.050  0.043 | 0.073  0.059  0.242  0.193  0.054
  n1_h3_v36_hd128  bf16  0.245  0.005  0.105  0.116  0.093 | 0.321  0.017  0.141  0.195  0.124
  n1_h1_v40_hd16   f32   0.009  0.005  0.023  0.021  0.022 | 0.019  0.018  0.060  0.064  0.028
  n1_h1_v40_hd16   bf16  0.167  0.004  0.091  0.085  0.079 | 0.273  0.007  0.148  0.117  0.099
  n2_h2_v44_hd96   f32   0.021  0.005  0.049  0.052  0.037 | 0.046  0.043  0.087  0.065  0.083
  n2_h2_v44_hd96   bf16  0.233  0.004  0.106  0.132  0.095 | 0.351  0.022  0.204  0.184  0.105
  n1_h1_v48_hd32   f32   0.019  0.006  0.030  0.048  0.031 | 0.031  0.022  0.070  0.089  0.037
  n1_h1_v48_hd32   bf16  0.196  0.005  0.088  0.093  0.104 | 0.367  0.013  0.119  0.124  0.095
  n1_h1_v52_hd16   f32   0.012  0.004  0.036  0.024  0.024 | 0.022  0.011  0.045  0.026  0.026
  n1_h1_v52_hd16   bf16  0.214  0.005  0.102  0.092  0.066 | 0.313  0.008  0.144  0.089  0.101
  n1_h2_v60_hd32   f32   0.016  0.005  0.055  0.049  0.032 | 0.042  0.026  0.049  0.055  0.048
  n1_h2_v60_hd32   bf16  0.191  0.006  0.097  0.117  0.095 | 0.285  0.013  0.164  0.171  0.114
  n1_h1_v64_hd16   f32   0.018  0.006  0.053  0.025  0.028 | 0.032  0.013  0.054  0.061  0.035
  n1_h1_v64_hd16   bf16  0.188  0.006  0.107  0.076  0.091 | 0.281  0.008  0.179  0.181  0.093
  n1_h1_v68_hd64   f32   0.025  0.005  0.041  0.036  0.049 | 0.035  0.025  0.074  0.078  0.045
  n1_h1_v68_hd64   bf16  0.187  0.005  0.081  0.097  0.086 | 0.279  0.011  0.142  0.126  0.112
  n2_h3_v132_hd32  f32   0.038  0.007  0.048  0.068  0.039 | 0.040  0.059  0.115  0.066  0.060
  n2_h3_v132_hd32  bf16  0.172  0.008  0.066  0.047  0.094 | 0.292  0.016  0.151  0.169  0.079
  n2_h1_v100_hd128 f32   0.060  0.007  0.066  0.058  0.077 | 0.125  0.070  0.155  0.162  0.096
  n2_h1_v100_hd128 bf16  0.187  0.007  0.121  0.109  0.104 | 0.353  0.017  0.116  0.128  0.092
  n1_h1_v216_hd96  f32   0.066  0.007  0.120  0.102  0.107 | 0.062  0.077  0.127  0.132  0.080
  n1_h1_v216_hd96  bf16  0.149  0.005  0.147  0.116  0.095 | 0.282  0.018  0.218  0.225  0.091
  n1_h1_v256_hd16  f32   0.026  0.006  0.051  0.055  0.044 | 0.027  0.020  0.072  0.051  0.054
  n1_h1_v256_hd16  bf16  0.137  0.007  0.100  0.144  0.065 | 0.289  0.008  0.216  0.291  0.086
  n1_h2_v1028_hd64 f32   0.064  0.012  0.070  0.071  0.081 | 0.079  0.060  0.136  0.116  0.113
  n1_h2_v1028_hd64 bf16  0.092  0.009  0.081  0.101  0.097 | 0.391  0.018  0.147  0.128  0.110
  largest          f32   0.125  0.077  0.242  0.193  0.113
  largest          bf16  0.391  0.022  0.250  0.386  0.161
The backward bounds are the project's 2e-4 (fp32) and 3e-2 (bf16) of max |ref| per block.  Against them fp32 stayed below 0.1 on every
case (largest 0.015: dQ of n1_h3_v36_hd128 at 4 / sqrt(hd)), so the fp32 bound is tightened to 4 x 0.015 x 2e-4 = 1.2e-5 and the fp32
figures above are fractions of that; bf16 reaches 0.39 and keeps 3e-2.  lse errs by at most 7.7e-6 in fp32 and 2.2e-6 in bf16.
The whole file takes 29 to 33 s on the MI355X (269 tests; the slowest 0.3 s).
"""
import pytest
import torch

import _attention_cases as AC
import _attention_ref as R
from _exact import assert_same_bits, in_sentinel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = {"f32": False, "bf16": True}
TD = {False: torch.float32, True: torch.bfloat16}
NAN = float("nan")


def _mods():
    from vdm4cdm_amd import _lib
    from vdm4cdm_amd import hip_ops
    return _lib, hip_ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Held:
    """A CPU tensor as a contiguous device view in the middle of a NaN-filled buffer, 256 bytes from either end."""

    def __init__(self, t, dtype):
        self.pad = 256 // torch.empty((), dtype=dtype).element_size()
        n = t.numel()
        self.buf = torch.full((n + 2 * self.pad,), NAN, dtype=dtype, device=DEV)
        self.t = self.buf[self.pad:self.pad + n].view(t.shape)
        self.t.copy_(t.to(dtype))
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()

    def ptr(self):
        return self.t.data_ptr()

    def around_is_nan(self):
        return bool(torch.isnan(self.buf[:self.pad]).all().item() and torch.isnan(self.buf[self.pad + self.t.numel():]).all().item())


def _out_view(shape, dtype):
    numel = 1
    for s in shape:
        numel *= s
    buf, view, ok = in_sentinel(numel, shape, pad=256 // torch.empty((), dtype=dtype).element_size(), dtype=dtype)
    assert view.data_ptr() % 16 == 0
    return buf, view, ok


class Launch:
    """The attention of one case the way a caller with its own buffers runs it: vdm_attn_fwd / vdm_attn_rowdot / vdm_attn_bwd directly,
    inputs held in NaN, outputs in sentinels.  q, k, v: [N, H, V, hd] fp32 on the CPU, already rounded to the storage type."""

    def __init__(self, case, bf16, q, k, v):
        _lib, self.ops = _mods()
        self.L, self.check = _lib.lib(), _lib.check
        self.case, self.bf16, self.dt, self.dt_id = case, bf16, TD[bf16], (_lib.VDM_BF16 if bf16 else _lib.VDM_F32)
        N, H, V, hd = case
        tr = lambda x: x.transpose(-1, -2).contiguous()
        self.q, self.k, self.v = (Held(x, self.dt) for x in (q, k, v))
        self.qt, self.kt, self.vt = (Held(tr(x), self.dt) for x in (q, k, v))
        self.out_buf, self.out, self.out_ok = _out_view((N, V, H * hd), self.dt)
        self.lse_buf, self.lse, self.lse_ok = _out_view((N, H, V), torch.float32)
        self.dqkv_buf, self.dqkv, self.dqkv_ok = _out_view((N, V, 3, H * hd), self.dt)

    def fwd(self, scale, want_lse=True):
        """-> out [N, H, V, hd], lse [N, H, V] on the CPU (fp32); without want_lse the lse buffer must stay as it was (NaN)."""
        N, H, V, hd = self.case
        self.out.fill_(NAN)
        self.lse.fill_(NAN)
        self.check(self.L.vdm_attn_fwd(self.q.ptr(), self.k.ptr(), self.vt.ptr(), N, V, H, hd, self.dt_id, float(scale), self.out.data_ptr(),
                                       self.lse.data_ptr() if want_lse else None, _stream()), "vdm_attn_fwd")
        torch.cuda.synchronize()
        assert self.out_ok() and self.lse_ok(), f"{self.case}: bytes around out / lse were written"
        lse = self.lse.cpu().clone()
        assert want_lse or bool(torch.isnan(lse).all()), f"{self.case}: lse written although it was not asked for"
        return AC.to_heads(self.out.float().cpu(), H), lse

    def bwd(self, dout, lse, dsum, scale, via_ops=False):
        """dout [N, V, H hd], lse [N, H, V], dsum [N, H, V] or None (then vdm_attn_rowdot of dout and the `out` of the last fwd), all on
        the CPU -> dQ, dK, dV [N, H, V, hd] on the CPU (fp32).  via_ops: through hip_ops.attn_bwd, which allocates dqkv itself."""
        N, H, V, hd = self.case
        doh = AC.to_heads(dout, H)
        hd_, ht, ho, hl = Held(doh, self.dt), Held(doh.transpose(-1, -2).contiguous(), self.dt), Held(dout, self.dt), Held(lse, torch.float32)
        hs = Held(torch.full((N, H, V), NAN) if dsum is None else dsum, torch.float32)
        if via_ops:
            dqkv = self.ops.attn_bwd(self.q.t, self.k.t, self.v.t, self.qt.t, self.kt.t, ho.t, self.out, hl.t, scale, dsum=None if dsum is None else hs.t)
            torch.cuda.synchronize()
        else:
            if dsum is None:
                self.check(self.L.vdm_attn_rowdot(ho.ptr(), self.out.data_ptr(), N, V, H, hd, self.dt_id, hs.ptr(), _stream()), "vdm_attn_rowdot")
            self.dqkv.fill_(NAN)
            self.check(self.L.vdm_attn_bwd(self.q.ptr(), self.k.ptr(), self.v.ptr(), self.qt.ptr(), self.kt.ptr(), hd_.ptr(), ht.ptr(), hl.ptr(), hs.ptr(),
                                           N, V, H, hd, self.dt_id, float(scale), self.dqkv.data_ptr(), _stream()), "vdm_attn_bwd")
            torch.cuda.synchronize()
            assert self.dqkv_ok() and self.out_ok(), f"{self.case}: bytes around dqkv were written"
            assert hs.around_is_nan(), f"{self.case}: bytes around dsum were written"
            dqkv = self.dqkv
        g = dqkv.float().cpu().reshape(N, V, 3, H * hd)
        return tuple(AC.to_heads(g[:, :, i].contiguous(), H) for i in range(3))


def _no_nan(case, **tensors):
    for name, t in tensors.items():
        assert not torch.isnan(t).any(), f"{case}: NaN in {name} (a load that left its tensor, or an element never written)"


CASES = pytest.mark.parametrize("case", AC.CASES, ids=AC.IDS)
BOTH = pytest.mark.parametrize("dtype", AC.DTYPES)


# =============================================================================================== A1: one-hot forward
@BOTH
@CASES
def test_onehot_forward(case, dtype):
    N, H, V, hd = case
    bf16 = BF[dtype]
    q, k, pi = AC.onehot_qk(case)
    v = AC.real_values(case, 11, bf16)
    run = Launch(case, bf16, q, k, v)
    out, lse = run.fwd(AC.ONEHOT_SCALE)
    _no_nan(case, out=out, lse=lse)
    assert_same_bits(out, R.take_rows(v, pi), f"{case}/{dtype}: out[n, h, i, d] vs v[pi(i)]")
    assert_same_bits(lse, torch.full((N, H, V), AC.ONEHOT_SCALE * hd), f"{case}/{dtype}: lse")
    out2, _ = run.fwd(AC.ONEHOT_SCALE, want_lse=False)
    assert torch.equal(out, out2), f"{case}/{dtype}: want_lse=False gives other bits"


# =============================================================================================== A2: uniform forward
@BOTH
@CASES
def test_uniform_forward(case, dtype):
    N, H, V, hd = case
    bf16 = BF[dtype]
    k, v = AC.real_values(case, 12, bf16), AC.int_values(case, 13)
    out, lse = Launch(case, bf16, torch.zeros(N, H, V, hd), k, v).fwd(1.0)
    _no_nan(case, out=out, lse=lse)
    ref = v.double().sum(2, keepdim=True).expand(N, H, V, hd) / V
    if V & (V - 1) == 0:
        assert_same_bits(out, R.storage(ref.float(), bf16), f"{case}/{dtype}: out vs column sum / V")
    else:
        excess = ((out.double() - ref).abs() - R.uniform_tol(ref, V, bf16)).max().item()
        assert excess <= 0, f"{case}/{dtype}: out leaves column sum / V by {excess} more than the roundings of 1 / V allow"


# =============================================================================================== A3, A4: one-hot backward
def _onehot_backward(case, bf16):
    N, H, V, hd = case
    q, k, pi = AC.onehot_qk(case)
    dout, v, dsum = AC.onehot_backward_operands(case, bf16)
    ref = R.onehot_backward(q, k, v, AC.to_heads(dout, H), dsum, pi, AC.ONEHOT_SCALE)
    assert max(r.abs().max().item() for r in ref) < 2 ** 24
    return Launch(case, bf16, q, k, v), dout, dsum, torch.full((N, H, V), AC.ONEHOT_SCALE * hd), [R.storage(r.float(), bf16) for r in ref]


@BOTH
@CASES
def test_onehot_backward_with_supplied_dsum(case, dtype):
    run, dout, dsum, lse, ref = _onehot_backward(case, BF[dtype])
    got = run.bwd(dout, lse, dsum, AC.ONEHOT_SCALE)
    _no_nan(case, dQ=got[0], dK=got[1], dV=got[2])
    for name, g, r in zip(("dQ", "dK", "dV"), got, ref):
        assert_same_bits(g, r, f"{case}/{dtype}: {name}[n, h, v, d]")
    for what, again in (("a second call", run.bwd(dout, lse, dsum, AC.ONEHOT_SCALE)),
                        ("hip_ops.attn_bwd(dsum=...)", run.bwd(dout, lse, dsum, AC.ONEHOT_SCALE, via_ops=True))):
        assert all(torch.equal(a, b) for a, b in zip(got, again)), f"{case}/{dtype}: {what} gives other bits"


@BOTH
@CASES
def test_onehot_backward_with_default_dsum(case, dtype):
    run, dout, _, lse, ref = _onehot_backward(case, BF[dtype])
    out, lse_dev = run.fwd(AC.ONEHOT_SCALE)                             # out = v[pi(i)]: dsum = dO_i . v_pi(i) = dP at the match
    assert torch.equal(lse_dev, lse)
    got = run.bwd(dout, lse, None, AC.ONEHOT_SCALE)
    _no_nan(case, dQ=got[0], dK=got[1], dV=got[2])
    assert_same_bits(got[0], torch.zeros_like(got[0]), f"{case}/{dtype}: dQ")
    assert_same_bits(got[1], torch.zeros_like(got[1]), f"{case}/{dtype}: dK")
    assert_same_bits(got[2], ref[2], f"{case}/{dtype}: dV")
    again = run.bwd(dout, lse, None, AC.ONEHOT_SCALE, via_ops=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), f"{case}/{dtype}: hip_ops.attn_bwd gives other bits than the direct calls"


# =============================================================================================== A5: head split
@BOTH
@CASES
def test_split_heads_copies_bits(case, dtype):
    _, ops = _mods()
    N, H, V, hd = case
    bf16, C = BF[dtype], H * hd
    for nsub in (1, 3):
        src = AC.real_values(case, 30 + nsub, bf16, (N, V, nsub * C))
        dev = Held(src, TD[bf16])
        for sub in range(nsub):
            want = AC.to_heads(src[:, :, sub * C:(sub + 1) * C].contiguous(), H)
            for rowmajor, transposed in ((True, True), (False, True), (True, False)):
                rm, tr = ops.attn_split_heads(dev.t, sub, nsub, H, rowmajor=rowmajor, transposed=transposed)
                what = f"{case}/{dtype} sub {sub} of {nsub} rowmajor={rowmajor} transposed={transposed}"
                assert (rm is None) == (not rowmajor) and (tr is None) == (not transposed), what
                if rowmajor:
                    assert rm.dtype == TD[bf16]
                    assert_same_bits(rm.float(), want, what + ": row-major [n, h, v, d]")
                if transposed:
                    assert tr.dtype == TD[bf16]
                    assert_same_bits(tr.float(), want.transpose(-1, -2), what + ": transposed [n, h, d, v]")


# =============================================================================================== A6: row dot
def _rowdot(case, bf16):
    _lib, _ = _mods()
    N, H, V, hd = case
    a, b = AC.int_values(case, 41, shape=(N, V, H * hd), terms=hd), AC.int_values(case, 42, shape=(N, V, H * hd), terms=hd)
    ha, hb = Held(a, TD[bf16]), Held(b, TD[bf16])
    buf, out, ok = _out_view((N, H, V), torch.float32)
    out.fill_(NAN)
    _lib.check(_lib.lib().vdm_attn_rowdot(ha.ptr(), hb.ptr(), N, V, H, hd, _lib.VDM_BF16 if bf16 else _lib.VDM_F32, out.data_ptr(), _stream()),
               "vdm_attn_rowdot")
    torch.cuda.synchronize()
    assert ok(), f"{case}: bytes around the row dots were written"
    ref = (a.long() * b.long()).reshape(N, V, H, hd).sum(-1).permute(0, 2, 1)
    assert_same_bits(out, ref, f"{case}: rowdot[n, h, v]")


@BOTH
@CASES
def test_rowdot_integers(case, dtype):
    _rowdot(case, BF[dtype])


def test_rowdot_grid_stride_loop():
    """N V H > 4096 x 256: the grid is capped at 4096 blocks and the first 16 threads take a second element."""
    _rowdot(AC.ROWDOT_GRID_STRIDE, True)


# =============================================================================================== A7: isolation
@BOTH
def test_samples_and_heads_are_isolated(dtype):
    case, bf16 = AC.ISOLATION_CASE, BF[dtype]
    N, H, V, hd = case
    scale = hd ** -0.5
    q, k, v, dout = AC.b_operands(case, bf16)
    full = Launch(case, bf16, q, k, v)
    out, lse = full.fwd(scale)
    grads = full.bwd(dout, lse, None, scale)
    _no_nan(case, out=out, lse=lse, dQ=grads[0], dK=grads[1], dV=grads[2])
    for n in range(N):
        for h in range(H):
            sl = lambda x: x[n:n + 1, h:h + 1].contiguous()
            one = Launch((1, 1, V, hd), bf16, sl(q), sl(k), sl(v))
            o1, l1 = one.fwd(scale)
            g1 = one.bwd(dout[n:n + 1, :, h * hd:(h + 1) * hd].contiguous(), l1, None, scale)
            for name, a, b in (("out", out, o1), ("lse", lse, l1), ("dQ", grads[0], g1[0]), ("dK", grads[1], g1[1]), ("dV", grads[2], g1[2])):
                assert_same_bits(sl(a), b, f"{dtype}: {name} of sample {n}, head {h} in the batch vs alone")


# =============================================================================================== B: random reals against float64
@BOTH
@CASES
def test_random_reals_against_float64(case, dtype):
    N, H, V, hd = case
    bf16 = BF[dtype]
    q, k, v, dout = AC.b_operands(case, bf16)
    doh = AC.to_heads(dout, H)
    run = Launch(case, bf16, q, k, v)
    failures = []
    for name, scale in AC.b_scales(hd):
        ref, rlse, P, A = R.ref_forward(q, k, v, scale)
        out, lse = run.fwd(scale)
        grads = run.bwd(dout, lse, None, scale)
        _no_nan(case, out=out, lse=lse, dQ=grads[0], dK=grads[1], dV=grads[2])
        err = (out.double() - ref).abs()
        r = {"out": (err / R.fwd_bound_bf16(A, ref)).max().item() if bf16 else err.max().item() / (R.FWD_F32 * ref.abs().max().item()),
             "lse": (lse.double() - rlse).abs().max().item() / R.LSE_TOL}
        for gname, g, rg in zip(("dQ", "dK", "dV"), grads, R.ref_backward(q, k, v, doh, P, scale, (doh.double() * ref).sum(-1))):
            r[gname] = (g.double() - rg).abs().max().item() / (R.BWD_TOL[bf16] * rg.abs().max().item())
        print(f"B {AC.IDS[AC.CASES.index(case)]} {dtype} {name}: err / bound " + "  ".join(f"{x} {y:.3f}" for x, y in r.items()))
        failures += [f"{name} {x}: {y:.3f} of the bound" for x, y in r.items() if not y <= 1.0]
    assert not failures, f"{case}/{dtype}: " + "; ".join(failures)
