"""Kernel-level parity tests of the forward and input-gradient convolutions, vdm_conv_fwd and vdm_conv_dgrad: every kernel plan_of()
picks between (csrc/conv_common.h; csrc/conv_fwd.hip: the generic kernel at its four tiles, its half-chunk SPLIT form, the rolling-z, the
K-split and the tap-packed kernel; csrc/conv_cls.hip: the three parity-class kernels), each through the C entry points with buffers of
its own.  The cases are in tests/_conv_cases.py; tests/test_conv_cpu.py confirms their plans, the reference and the bound of check B
without a device.  Every case asserts its plan (vdm_conv_plan) before it launches.

Every launch: the packed weights get exactly the plan's packed_bytes inside a guarded buffer; the output is a view inside a sentinel
buffer and all NaN before the call; the staged tensor and the residual are views inside NaN-filled buffers (a halo or tail read that
strays outside the tensor and is used poisons the result), the padding channels of the staged tensor are zero as the ABI says; the
per-sample bias is a column block of a wider NaN-filled table.  After every call: status 0, no sentinel changed, no NaN in the output,
a second call gives the same bits.

Three kinds of check:
  A. exact integers, no tolerance.  Activations / dout, master weights and residual are small integers in the storage type, bias and
     per-sample bias integers in [-8, 8]: every product and partial sum is an integer below 2^24, fp32 addition is exact in any order,
     and the output must have the BITS of the float64 reference (tests/_conv_ref.py) rounded ONCE to the output type - a dropped,
     duplicated or mis-wrapped voxel, a wrong channel of one tap on one tile face, a padded voxel read as circular all show, and
     assert_same_bits reports where.  Every case runs with integers in {-2..2} and again in {0..3}: the biased sums reach ~2.25 x 27 x
     cin, far above 256, so a bf16 output is a genuine round-to-nearest-even of an integer, and a kernel that rounds twice, truncates
     or carries a partial sum in less than fp32 shows.  Variants: plain; forward with bias + strided per-sample bias + residual (the
     up-sampling conv takes no per-sample bias); dgrad with the residual it accumulates gradients into.  One forward case per family
     also runs with gn_partials requested: the output keeps its bits (the partials themselves are test_groupnorm_kernels_gpu.py's).
  B. random reals against the float64 reference, operands rounded to the storage type first, per element
         |out - ref| <= (eps_op + L * 2^-24) * abs_sum + eps_merge * abs_conv + store(ref) + 2^-126
     with eps_op the error of one product (0 for bf16 storage; 3.01 * 2^-18 for fp32 storage on the bf16 pipe, 2^-24 in the
     VDM4CDM_FP32_EXACT build), L the fp32 additions one product passes through (MFMA chain over taps and K-blocks, the K-split fold,
     the eight classes of the up-conv dgrad, the epilogue terms), eps_merge the rounding of a merged class weight - all derived per
     kernel from the code and computed from the plan of the launch (_conv_ref.py depth, eps_merge), never fitted.
  C. refusals stay refusals: status != 0 and the output still all NaN.

B, measured max over the elements of err / bound on an MI355X, default build (case, family, L, ratio), full epilogue:
  g_1x4_ragged_circ_fwd        GENERIC           62   0.971
  g_1x8_fwd                    GENERIC           62   0.991
  g_2x8_dgrad                  GENERIC           60   0.990
  roll_equal_segments_fwd      GENERIC           62   0.991
  roll_unequal_segments_dgrad  GENERIC           60   0.991
  g_nc4_4x8_fwd                GENERIC           89   0.989
  split_1x4_fwd                SPLIT             89   0.968
  split_1x8_dgrad              SPLIT             87   0.984
  split_2x8_fwd                SPLIT             89   0.987
  g_partial_24_40_dgrad        GENERIC           87   0.963
  ksplit_ty4_fwd               KSPLIT            64   0.985
  ksplit_5kb_circ_fwd          KSPLIT            91   0.968
  ksplit_ty8_dgrad             KSPLIT            62   0.987
  kpack_2_32_fwd               KPACK             42   0.985
  kpack_3_16_circ_fwd          KPACK             42   0.991
  kpack_conv_out_dgrad         KPACK             40   0.992
  g_nc1_fwd                    GENERIC           62   0.984
  g_conv_out_f32_fwd           GENERIC           62   0.011
  f32_20_24_circ_fwd           GENERIC          181   0.045      (VDM4CDM_FP32_EXACT build: L = 871, 0.004)
  f32_20_24_circ_dgrad         GENERIC          179   0.049      (VDM4CDM_FP32_EXACT build: L = 869, 0.004)
  k1_64_32_fwd                 GENERIC           37   0.991
  k1_64_32_f32_dgrad           GENERIC           23   0.513      (VDM4CDM_FP32_EXACT build: L = 37, 0.109)
  s2_32_64_fwd                 GENERIC           62   0.974
  s2_32_64_f32_fwd             GENERIC          181   0.046      (VDM4CDM_FP32_EXACT build: L = 871, 0.005)
  s2_32_64_dgrad               CLASS/S2_DGRAD    49   0.990
  s2_32_64_f32_dgrad           CLASS/S2_DGRAD   113   0.184      (VDM4CDM_FP32_EXACT build: L = 517, 0.006)
  ups_32_16_fwd                CLASS/UP_FWD      42   0.289
  ups_64_32_fwd                CLASS/UP_FWD      50   0.321
  ups_128_64_fwd               CLASS/UP_FWD      66   0.250
  ups_64_32_f32_fwd            CLASS/UP_FWD     114   0.051      (VDM4CDM_FP32_EXACT build: L = 518, 0.004)
  ups_64_32_dgrad              CLASS/UP_DGRAD    97   0.066
  ups_16_32_dgrad              CLASS/UP_DGRAD    97   0.075
  ups_64_32_f32_dgrad          CLASS/UP_DGRAD   401   0.011      (VDM4CDM_FP32_EXACT build: L = 2053, 0.001)
  (a bf16 output is dominated by store(ref): the largest rounding of the store over 10^4 - 10^6 elements comes within a few percent of
  half an ulp, which is what the ratios near 0.99 are - the fp32 emulation of tests/test_conv_cpu.py gives the same figures; the fp32
  outputs show the accumulation alone, a worst case over the signs of L roundings against random roundings that err like sqrt(L).  The
  emulated faults of tests/test_conv_cpu.py exceed the same bounds 40 to 300 000 times, a wrong merged tap of one class entry of the
  bf16 up-sampling conv 12 to 16 times forward and 1.6 to 1.8 times in its input gradient, where the 2^-8 of the re-rounded merged
  weights is the bound's largest term.)
"""
import ctypes

import pytest
import torch

import _conv_cases as W
import _conv_ref as R
from _exact import assert_same_bits, in_sentinel, ints, ints_biased

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                          # bytes around the packed weights (0xFF: a NaN in either storage type): not written, and poison if read
PAD = 64                              # elements around the NaN-framed operands
DISTS = {"signed": ints, "biased": ints_biased}
NAN = float("nan")


def _lib():
    from vdm4cdm_amd import _lib as lib
    return lib


def _framed(t, dtype, cpad=None):
    """[..., c] fp32 on the CPU -> a contiguous [..., cpad] view in `dtype` on the device in the middle of a NaN-filled buffer; the
    padding channels are zero."""
    cpad = cpad or t.shape[-1]
    shape = tuple(t.shape[:-1]) + (cpad,)
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + 2 * PAD,), NAN, dtype=dtype, device=DEV)
    view = buf[PAD:PAD + numel].view(shape)
    view.zero_()
    view[..., :t.shape[-1]] = t.to(dtype).to(DEV)
    return buf, view


class Launch:
    """One vdm_conv_fwd / vdm_conv_dgrad launch of a case the way a caller with its own buffers makes it."""

    def __init__(self, c, xin, w, expect_ok=True):
        lib = _lib()
        from vdm4cdm_amd import hip_ops as ops
        self.c, self.L = c, lib.lib()
        self.dgrad = int(c.direction == "dgrad")
        self.d = W.desc_of(c)
        self.info = lib.ConvPlanInfo()
        st = self.L.vdm_conv_plan(self.d, self.dgrad, ctypes.byref(self.info))
        if expect_ok:
            assert st == 0, self.L.vdm_last_error()
            W.assert_plan(c, self.info)                                  # the case is wrong if the plan says otherwise
        self.stream = torch.cuda.current_stream().cuda_stream
        # packed weights: exactly packed_bytes, guarded
        self.need = self.info.packed_bytes
        assert self.need == self.L.vdm_conv_packed_bytes(self.d, self.dgrad) and self.need > 0
        self.wbuf = torch.full((self.need + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.wp = self.wbuf[GUARD:GUARD + self.need]
        self.wm = w.to(DEV).contiguous()
        st = self.L.vdm_conv_pack_weights(self.d, self.dgrad, self.wm.data_ptr(), self.wp.data_ptr(), self.stream)
        torch.cuda.synchronize()
        assert st == 0, self.L.vdm_last_error()
        assert self.guards_ok(), f"{c.name}: the packer wrote outside packed_bytes"
        self.xbuf, self.x = _framed(xin, c.dtype, ops.cpad(W.K(c), c.dtype))
        self.out_buf, self.out, self.out_ok = in_sentinel(self.numel(W.out_shape(c)), W.out_shape(c), dtype=W.out_dtype(c))
        self.keep = []

    @staticmethod
    def numel(shape):
        n = 1
        for s in shape:
            n *= s
        return n

    def guards_ok(self):
        return bool((self.wbuf[:GUARD] == 0xFF).all()) and bool((self.wbuf[GUARD + self.need:] == 0xFF).all())

    def call(self, bias=None, nbias=None, res=None, gn=False, null=()):
        """One call with the output all NaN before it; returns the status.  null: arguments passed as NULL."""
        c = self.c
        self.out.fill_(NAN)
        ptr = lambda name, t: None if (t is None or name in null) else t.data_ptr()      # noqa: E731
        rv = _framed(res, c.dtype)[1] if res is not None else None
        self.gnp = None
        if self.dgrad:
            st = self.L.vdm_conv_dgrad(self.d, ptr("x", self.x), ptr("w", self.wp), ptr("res", rv), ptr("out", self.out), self.stream)
        else:
            bd = bias.to(DEV) if bias is not None else None
            nb_ptr, nstride, tab = None, 0, None
            if nbias is not None:
                co = nbias.shape[1]
                nstride = co + W.NBIAS_STRIDE_EXTRA
                tab = torch.full((c.n, nstride), NAN, device=DEV)
                tab[:, 2:2 + co] = nbias.to(DEV)
                nb_ptr = tab.data_ptr() + 2 * 4
            if gn:
                self.gnp_buf, self.gnp, self.gnp_ok = in_sentinel(c.n * self.info.tiles * c.cout * 2, (c.n, self.info.tiles, c.cout, 2))
                self.gnp.fill_(NAN)
            st = self.L.vdm_conv_fwd(self.d, ptr("x", self.x), ptr("w", self.wp), ptr("bias", bd), nb_ptr, nstride, ptr("res", rv),
                                     ptr("out", self.out), None if self.gnp is None else self.gnp.data_ptr(), self.stream)
            self.keep = [bd, tab]
        torch.cuda.synchronize()
        self.keep.append(rv)
        return st

    def run(self, **kw):
        """A call that must succeed, twice; returns the output on the CPU."""
        c = self.c
        outs = []
        for _ in range(2):
            st = self.call(**kw)
            assert st == 0, self.L.vdm_last_error()
            assert self.guards_ok(), f"{c.name}: bytes around the packed weights were written"
            assert self.out_ok(), f"{c.name}: bytes around the output were written"
            if self.gnp is not None:
                assert self.gnp_ok() and not torch.isnan(self.gnp).any(), f"{c.name}: gn_partials: sentinel changed or a slot not written"
            o = self.out.cpu().clone()
            assert not torch.isnan(o).any(), f"{c.name}: NaN in the output (a voxel not written, or a read outside the tensor)"
            outs.append(o)
        assert torch.equal(outs[0], outs[1]), f"{c.name}: a second call gives other bits"
        return outs[0]


def _work(c):
    return Launch.numel(W.oshape(c)) * c.ks ** 3 * c.cin * c.cout


# =============================================================================================== A: exact integers
@pytest.mark.parametrize("dist", list(DISTS), ids=list(DISTS))
@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_conv_exact_integers(case, dist):
    c, mk = case, DISTS[dist]
    nt = W.terms(c)
    xin, w = mk(W.in_shape(c), 11, nt), mk((c.ks ** 3, c.cout, c.cin), 12, nt)
    bias, nbias, res = W.epilogue_operands(c, 13, real=False)
    # float32 has the float64 bits here (test_conv_cpu.py test_fp32_reference_has_the_float64_bits_on_integers): the large grids use it
    plain = W.ref(c, xin, w, dtype=torch.float32 if _work(c) > 2e9 else torch.float64, want_abs=False)[0].double()
    full = R.add_epilogue(plain, None, bias, nbias, res)[0]
    assert full.abs().max().item() < 2 ** 24 and plain.abs().max().item() < 2 ** 24
    once = lambda t: t.to(W.out_dtype(c)).double()                                   # noqa: E731  one rounding to the output type
    run = Launch(c, xin, w)
    tag = f"{c.name}/{dist}"
    got = run.run()
    assert got.dtype == W.out_dtype(c)
    assert_same_bits(got, once(plain), f"{tag}: plain [n, z, y, x, channel]")
    got_full = run.run(bias=bias, nbias=nbias, res=res)
    assert_same_bits(got_full, once(full), f"{tag}: with bias / per-sample bias / residual [n, z, y, x, channel]")
    if c.name in W.GN_CASES:
        assert torch.equal(run.run(gn=True), got), f"{tag}: gn_partials requested: other output bits"
        assert torch.equal(run.run(bias=bias, nbias=nbias, res=res, gn=True), got_full), f"{tag}: gn_partials with the epilogue terms"


# =============================================================================================== B: random reals, derived bound
@pytest.mark.parametrize("name", W.B_CASES)
def test_conv_random_reals_within_derived_bound(name):
    lib = _lib()
    c = W.BY_NAME[name]
    xin, w = W.real_operands(c, 7)
    bias, nbias, res = W.epilogue_operands(c, 8, real=True)
    run = Launch(c, xin, w)
    got = run.run(bias=bias, nbias=nbias, res=res).double()
    bf16 = c.dtype == W.BF
    fam, kind = W.family_of(run.info), W.cls_kind_of(run.info)
    L = W.depth(c, run.info, lib.FP32_EXACT)
    plain, abs_conv = W.ref(c, xin, w)
    ref, abs_sum = R.add_epilogue(plain, abs_conv, bias, nbias, res)
    bnd = R.bound(ref, abs_sum, abs_conv, L, R.eps_op(bf16, lib.FP32_EXACT), R.eps_merge(fam, kind, bf16), W.out_dtype(c) == W.BF)
    ratio = ((got - ref).abs() / bnd).max().item()
    msg = f"B {name:30s} {fam + ('/' + kind if kind else ''):15s} L = {L:4d}  max err / bound = {ratio:.3f}"
    print(msg)
    assert ratio <= 1.0, msg


# =============================================================================================== C: refusals
def _refused(c, **kw):
    nt = W.terms(c)
    run = Launch(c, ints(W.in_shape(c), 1, nt), ints((c.ks ** 3, c.cout, c.cin), 2, nt), expect_ok=False)
    st = run.call(**kw)
    assert st != 0, f"{c.name}: the call was accepted"
    assert bool(torch.isnan(run.out).all()) and run.out_ok(), f"{c.name}: a refused call wrote the output"
    return run.L.vdm_last_error()


@pytest.mark.parametrize("what,kw", [("cout_32", dict(cout=32)), ("ksize_1", dict(ks=1)), ("stride_2", dict(stride=2))])
def test_out_f32_is_refused_outside_conv_out(what, kw):
    assert b"out_f32" in _refused(W.BY_NAME["g_conv_out_f32_fwd"]._replace(**kw))


def test_upsampling_conv_refuses_per_sample_bias_and_out_f32():
    c = W.BY_NAME["ups_32_16_fwd"]
    assert b"up-sampling" in _refused(c, nbias=torch.zeros(c.n, c.cout))
    assert b"up-sampling" in _refused(c._replace(out_f32=True))


@pytest.mark.parametrize("name", ["g_1x4_ragged_fwd", "g_1x4_ragged_dgrad", "ups_32_16_fwd", "s2_32_64_dgrad"])
@pytest.mark.parametrize("null", ["x", "w", "out"])
def test_null_pointers_are_refused(name, null):
    assert b"NULL" in _refused(W.BY_NAME[name], null=(null,))
