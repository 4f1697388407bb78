"""Kernel-level parity tests of K6, csrc/cond.hip: the conditioning MLPs and the additive injection table of all ResNet blocks
(vdm_cond_table_fwd, the three kernels of vdm_cond_table_bwd, K6i vdm_cond_input_grad, the sampler's vdm_cond_table_step), each through
the C entry points with buffers of its own.  The cases are in tests/_cond_cases.py, each named for the code edge it sits on;
tests/test_cond_cpu.py confirms those edges, the references, the bound and what emulated faults do to the checks without a device.

Every launch: `table`, `saved` (exactly vdm_cond_saved_floats), `scratch` (exactly vdm_cond_bwd_scratch_floats), every gradient tensor
(dw1, db1, dw2, db2, dwproj, dbias) and every dinputs[k] is a view inside a sentinel buffer (_exact.in_sentinel) and all NaN before the
call; inputs and weights are views inside NaN-filled buffers; dtable is a column block of a wider NaN-filled matrix (dtable_stride >
width).  A weight matrix whose row length is a multiple of 4 sits 16-byte aligned, as the contract asks; where the contract does not ask
(in_dim % 4 != 0 for w1, dim % 4 != 0 for w2 and wproj) it sits at an address that is 4-byte and not 16-byte aligned, so the scalar path
really is the one taken.  After every call: status 0, no sentinel changed, no NaN in any output (every element was written, nothing
outside a tensor was read and used), a second call gives the same bits.  saved == NULL gives the same table bits, dbias == NULL the
same parameter gradients, a NULL entry of dinputs leaves the others bit-equal.

Three kinds of check, both A and B on every case:
  A. exact, no tolerance.  For fp32 |x| >= 16, erff(x / sqrt 2) is exactly +-1 and __expf(-x^2 / 2) exactly 0 (exp(-128) lies 11 decades
     below the smallest denormal), so gelu_f(x) = max(x, 0) and dgelu_f(x) = 1 or 0 exactly; at x = 0 they give 0 and 1/2.  Vector
     conditionings with inputs in {-2..2}, w1 and b1 multiples of 16, w2 / wproj / dtable small integers, b2 a multiple of 16 put every
     pre-activation at 0 or beyond +-16: the forward is exact integer arithmetic, the backward exact in quarter-integers, and the table,
     all four parts of `saved`, the (dh1, dh2) rows of `scratch`, every parameter gradient, dbias and the vector dinputs must have the
     BITS of an int64 reference that uses ReLU with slope 1/2 at 0 and never calls erf (_cond_ref.ref_int).  A sinusoidal conditioning
     joins at t = 0, where the embedding is exactly [0..0, 1..1] (its dL/dt carries 1000 f_i and is check B's).  The reference asserts
     on the CPU that every sum of magnitudes stays below 2^22 (exact in any order), that every column of every weight matrix carries a
     nonzero, that h1 and h2 each show > 0, == 0 and < 0, and that the backward half compares no 0 with 0: every backward tensor holds
     a nonzero, in both layers an element with h == 0 meets a nonzero gradient, and somewhere gelu'(h1) != gelu'(h2) under one.
     The precondition c == max(h2, 0) is asserted on its own from `saved`: a failure there would be a finding about the device's
     erff, not about indexing.
  B. random reals against float64 (_cond_ref.ref64), per element |device - ref| <= bound with u = 2^-24, the bound counted from the code
     per case (_cond_ref.bounds), never fitted:
       - the saved embedding is checked on its own against float64 sin / cos(1000 t f_i): |arg| u (K_FREQ + 2) + K_SINCOS u |result|
         (the relative error of the device's f - two roundings in expf's argument, about 2 * 9.21 u, and expf - the two products of
         1000 * t * f, all times |arg| <= 1000: about 1e-3 at t = 1; then sinf / cosf).  Everything behind it starts from the saved
         embedding, read back and given to the float64 reference as the MLP's input, so that 1e-3 never enters the table or the
         gradients.
       - a dot product of length len shared by tpo lanes: n = the busiest lane's fmas (4 per 16-byte quad of its stride, then its share
         of the scalar tail: _cond_cases.chain) + log2 tpo butterfly additions + the bias addition; error gamma_n (|b| + sum |w||x|)
         + sum |w| |dx| for the error dx the input already carries, gamma_n = n u / (1 - n u).
       - GELU adds sup|gelu'| |dh| + E_gelu(h), sup|gelu'| = 1.129; E_gelu(h) = |h| / 2 * u (K_ERF |erf z| + 2 |z| erf'(z) + (1 + erf z))
         + u |gelu(h)|, z = h / sqrt 2: erff, the rounded constant and product in its argument, the addition, the last product.
       - the table adds gamma_(n - 1) sum |c||wproj| for the n - 1 additions over the conditionings.
       - backward: the slab partials are chains of ceil(min(32, width) / nws) fmas plus the LDS fold over nws, the fold over the slabs a
         chain of ceil(nslab / nws) additions plus the LDS fold over nws; the product with gelu' rounds once and carries
         |dc| (sup|gelu''| |dh| + E_dgelu(h)), sup|gelu''| = 0.798; E_dgelu(h) = the erf half as above + |h| phi(h) u (3 h^2 / 2 + 7)
         (__expf after _gn_bounds.silu_eval_err's model, its argument's rounding, the constant, two products) + u |gelu'(h)|; dh1 the
         same behind a chain of ceil(dim / nws) + nws.  The parameter gradients are chains of `rows` fmas over operands that carry
         the errors above (dw2 holds a re-evaluated gelu_f(h1): E_a1 again).
       - K6i: the dim-long chain; for dL/dt the factors 1000 f_i (relative (K_FREQ + 3) u with the products), the saved sin and cos,
         and the 8-level LDS tree: a bound in sums of magnitudes, the honest scale of that cancelling sum.  The reference takes the
         saved sin and cos as they are (the function differentiated is the one the forward evaluated).
  C. refusals stay refusals (tests/test_cond_cpu.py, on the host); here one refused forward and one refused backward leave every output
     all NaN.  vdm_cond_table_step is bit-exact in its four sub-cases.

Library errors, measured on an MI355X against float64 (test_library_errors), in u |result| (and ulp of the result); constant = 4 x:
  erff, through the (h2, c) pairs of `saved`, all of gelu_f's error charged to it:  5.418 (4.434 ulp) over 12607 pairs    K_ERF    = 21.67
  sinf / cosf, exact arguments 1000 m 2^-14 <= 1000:                               1.932 (1.460 ulp) over 32768 values   K_SINCOS =  7.73
  f_i = expf(-ln 1e4 i / half), through sin(1000 * 2^-20 f_i), half = 1..128:      20.257 relative over 8256 (i, half)   K_FREQ   = 81.03
  None is above 8 ulp of the result (the 4.4 ulp of erff hold the four other roundings of gelu_f as well).  erff is measured over
  0.5 <= |x| <= 6 only: below 0.5 its relative error cannot be told from the rounding of 1 + erf, and K_ERF is ASSUMED to hold there,
  not measured.  What the bound uses is the whole model E_gelu, and that is held against the device over all of |x| <= 6, the
  1207 pairs below 0.5 included: worst |gelu_f - gelu64| / E_gelu = 0.699.  test_library_errors also fails when
  a measured value leaves [1 / 1.5, 1.5] x the recorded one, so that these figures cannot go stale unseen.

B, measured max over the elements of err / bound, MI355X / fp32 emulation of tests/_cond_ref.py (emb: the embedding's own check).  The
emulation column is the one of the host that ran beside the device: it goes through that host's erf, exp, sin and cos in torch, so
another CPU gives figures that differ in the second digit (c of v3_65: 0.018 here, 0.012 elsewhere); that is no drift.
  case         table       h1          h2          c           dh2         dh1         dw1         db1         dw2         db2         dwproj      dbias       din
  v1_3         0.002/0.001 0.101/0.101 0.058/0.058 0.027/0.027 0.040/0.040 0.048/0.014 0.044/0.009 0.046/0.019 0.039/0.022 0.008/0.016 0.024/0.024 0.174/0.174 0.015/0.015
  v3_65        0.002/0.002 0.322/0.322 0.027/0.027 0.018/0.018 0.035/0.035 0.022/0.021 0.004/0.003 0.003/0.003 0.025/0.025 0.012/0.012 0.013/0.012 0.348/0.348 0.001/0.001
  v6_64        0.002/0.002 0.332/0.332 0.019/0.019 0.013/0.013 0.036/0.036 0.023/0.042 0.003/0.007 0.002/0.004 0.031/0.031 0.011/0.011 0.013/0.007 0.183/0.183 0.001/0.001
  v4_128       0.001/0.001 0.311/0.311 0.017/0.016 0.010/0.010 0.015/0.014 0.008/0.026 0.003/0.003 0.002/0.002 0.018/0.014 0.008/0.008 0.010/0.011 0.359/0.359 0.000/0.000
  v252_132     0.000/0.000 0.009/0.009 0.001/0.001 0.000/0.000 0.005/0.005 0.001/0.001 0.000/0.000 0.000/0.000 0.003/0.003 0.002/0.002 0.000/0.000 0.497/0.497 0.000/0.000
  v256_256     0.000/0.000 0.010/0.010 0.000/0.000 0.000/0.000 0.002/0.002 0.001/0.001 0.000/0.000 0.000/0.000 0.001/0.001 0.000/0.000 0.000/0.000 0.553/0.553 0.000/0.000
  t64_64_v6_64 0.001/0.001 0.269/0.269 0.018/0.018 0.016/0.016 0.009/0.009 0.015/0.015 0.003/0.003 0.001/0.001 0.008/0.008 0.005/0.004 0.022/0.022 0.511/0.511 0.001/0.000  emb 0.149/0.104
  four_mlps    0.000/0.000 0.253/0.253 0.123/0.123 0.032/0.032 0.026/0.026 0.028/0.028 0.017/0.014 0.006/0.006 0.022/0.022 0.009/0.010 0.048/0.045 0.429/0.429 0.009/0.007  emb 0.012/0.012
  t256_64      0.000/0.000 0.007/0.007 0.001/0.001 0.000/0.000 0.002/0.002 0.001/0.001 0.001/0.001 0.001/0.001 0.003/0.004 0.002/0.002 0.000/0.000 0.000/0.000 0.000/0.000  emb 0.146/0.107
  t6_16        0.009/0.009 0.311/0.311 0.045/0.058 0.030/0.036 0.044/0.040 0.047/0.031 0.008/0.006 0.005/0.005 0.021/0.023 0.012/0.012 0.020/0.020 0.214/0.214 0.002/0.001  emb 0.050/0.050
  (the bound is a worst case over the signs of every rounding and of every term of the sums; random roundings err like the square root
  of both counts, which is what the ratios of 0.001 - 0.05 behind the long sums are.  dbias and h1, short chains over few terms, come
  closest.)

What each emulated fault does to A and to B (tests/_cond_ref.py emulate(fault=...), asserted by tests/test_cond_cpu.py) over the ten
cases: cases in which check A's bits break / cases in which bound
B is exceeded, and the range of the worst err / bound over the latter:
  last element of a dot product dropped         A 10  B 10   870 .. 3.6e6
  scalar tail dropped (len % 4 != 0)            A  6  B  6   2.2e6 .. 4.1e6      (the six cases with such a length; none elsewhere)
  forward slab boundary off by one              A  7  B  7   inf (an unwritten column)   (the cases with width >= 64)
  backward slab boundary off by one             A 10  B 10   1.7e3 .. 7.2e5
  second fold pass dropped                      A  3  B  3   3.6e3 .. 1.4e4      (the three cases that have one)
  dgelu taken at h1 where h2 belongs            A 10  B 10   1.2e3 .. 8.3e5
  the 1/2 at 0 missing                          A 10  B  0   -                   (random reals never hit 0: check A alone sees it)
  tanh approximation in place of erf            A  0  B 10   1.8 .. 398          (the tanh form saturates like erf: bound B alone)
  saved offset of mlp k with mlp 0's sizes      A  1  B  1   inf                 (the case with uneven sizes)
  dtable read with stride width                 A  9  B  9   inf (a NaN of the frame is read)   (every case with rows > 1)
  sin and cos halves exchanged                  A  4  B  4   1.5e6 ..            (the four cases with a sinusoid)
  i / (half - 1) in the frequency law           A  1  B  4   1.3e4 .. inf        (check A runs at t = 0: the embedding check of B)
"""
import ctypes

import pytest
import torch

import _cond_cases as W
import _cond_ref as R
from _exact import assert_same_bits, in_sentinel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64                              # elements around the NaN-framed operands (256 bytes: the views keep the buffer's alignment)
NAN = float("nan")
DT_LEFT, DT_RIGHT = 2, 3              # NaN columns left and right of dtable inside its wider matrix
U = R.U


def _lib():
    from vdm4cdm_amd import _lib as lib
    return lib


def _framed(t, misalign=False):
    """fp32 CPU tensor -> a contiguous device view in the middle of a NaN-filled buffer.  The view starts 16-byte aligned, or - for a
    weight matrix whose rows the contract does not ask to be aligned - at an address that is 4-byte and not 16-byte aligned."""
    n = t.numel()
    buf = torch.full((n + 2 * PAD + 4,), NAN, dtype=torch.float32, device=DEV)
    off = PAD + (1 if misalign else 0)
    view = buf[off:off + n].view(t.shape)
    view.copy_(t.float())
    assert view.data_ptr() % 16 == (4 if misalign else 0)
    return buf, view


class Launch:
    """The K6 calls of one set of operands the way a caller with its own buffers makes them."""

    def __init__(self, ops):
        lib = _lib()
        self.L, self.ops = lib.lib(), ops
        self.rows, self.width, self.n = ops["rows"], ops["width"], len(ops["mlps"])
        self.stream = torch.cuda.current_stream().cuda_stream
        self.keep, self.checks, self.outs = [], [], {}
        self.arr = (lib.CondMlp * self.n)()

        def out(key, shape):
            numel = 1
            for s in shape:
                numel *= s
            buf, view, ok = in_sentinel(numel, shape)
            self.keep.append(buf)
            self.checks.append((key, ok))
            self.outs[key] = view
            return view

        for k, m in enumerate(ops["mlps"]):
            d = self.arr[k]
            d.in_dim, d.dim, d.sinusoid = m["in_dim"], m["dim"], int(m["sinusoid"])
            for name, mis in (("input", False), ("w1", m["in_dim"] % 4 != 0), ("b1", False), ("w2", m["dim"] % 4 != 0), ("b2", False),
                              ("wproj", m["dim"] % 4 != 0)):
                buf, view = _framed(m[name], mis)
                self.keep.append(buf)
                setattr(d, name, view.data_ptr())
            for name in ("w1", "b1", "w2", "b2", "wproj"):
                setattr(d, "d" + name, out(f"{k}.d{name}", tuple(m[name].shape)).data_ptr())
            out(f"{k}.din", tuple(m["input"].shape))
        out("table", (self.rows, self.width))
        out("dbias", (self.width,))
        self.saved_floats = self.L.vdm_cond_saved_floats(self.arr, self.n, self.rows)
        self.scratch_floats = self.L.vdm_cond_bwd_scratch_floats(self.arr, self.n, self.rows, self.width)
        out("saved", (self.saved_floats,))
        out("scratch", (self.scratch_floats,))
        self.stride = DT_LEFT + self.width + DT_RIGHT
        wide = torch.full((self.rows * self.stride + 2 * PAD,), NAN, dtype=torch.float32, device=DEV)
        self.keep.append(wide)
        self.dtable = wide[PAD:PAD + self.rows * self.stride].view(self.rows, self.stride)[:, DT_LEFT:DT_LEFT + self.width]
        self.dtable.copy_(ops["dtable"])
        assert self.dtable.stride(0) > self.width

    # ---- the calls; each returns the status
    def nan(self, *keys):
        for key in (keys or self.outs):
            self.outs[key].fill_(NAN)

    def fwd(self, save=True):
        return self.L.vdm_cond_table_fwd(self.arr, self.n, self.rows, self.width, self.outs["table"].data_ptr(),
                                         self.outs["saved"].data_ptr() if save else None, self.stream)

    def bwd(self, dbias=True, stride=None):
        return self.L.vdm_cond_table_bwd(self.arr, self.n, self.rows, self.width, self.dtable.data_ptr(), self.stride if stride is None else stride,
                                         self.outs["saved"].data_ptr(), self.outs["scratch"].data_ptr(),
                                         self.outs["dbias"].data_ptr() if dbias else None, self.stream)

    def din(self, want=None):
        want = [True] * self.n if want is None else want
        ptrs = (ctypes.c_void_p * self.n)(*[self.outs[f"{k}.din"].data_ptr() if w else None for k, w in enumerate(want)])
        return self.L.vdm_cond_input_grad(self.arr, self.n, self.rows, self.width, self.outs["saved"].data_ptr(),
                                          self.outs["scratch"].data_ptr(), ptrs, self.stream)

    def all_calls(self):
        self.nan()
        assert self.fwd() == 0, self.L.vdm_last_error()
        assert self.bwd() == 0, self.L.vdm_last_error()
        assert self.din() == 0, self.L.vdm_last_error()
        torch.cuda.synchronize()
        return self.raw()

    def raw(self):
        return {key: v.detach().cpu().clone() for key, v in self.outs.items()}

    def untouched(self):
        bad = [key for key, ok in self.checks if not ok()]
        assert not bad, f"a sentinel around {bad} has changed: a kernel wrote outside the tensor"

    def unpack(self, raw):
        """`saved` and `scratch` by the layout the ABI states -> the keys of _cond_ref."""
        out = {key: v for key, v in raw.items() if key not in ("saved", "scratch")}
        so = co = 0
        for k, m in enumerate(self.ops["mlps"]):
            i_d, d = m["in_dim"], m["dim"]
            sv = raw["saved"][so:so + self.rows * (i_d + 3 * d)].view(self.rows, i_d + 3 * d)
            sc = raw["scratch"][co:co + self.rows * 2 * d].view(self.rows, 2 * d)
            so, co = so + sv.numel(), co + sc.numel()
            out.update({f"{k}.emb": sv[:, :i_d], f"{k}.h1": sv[:, i_d:i_d + d], f"{k}.h2": sv[:, i_d + d:i_d + 2 * d], f"{k}.c": sv[:, i_d + 2 * d:],
                        f"{k}.dh1": sc[:, :d], f"{k}.dh2": sc[:, d:]})
        return out


def _same(a, b, keys, what):
    for key in keys:
        assert_same_bits(a[key], b[key], f"{what}: {key}")


def run_framed(ops, variants=True):
    """All calls of one set of operands with every framing assertion of the module; returns the unpacked outputs."""
    ln = Launch(ops)
    assert ln.saved_floats == sum(ops["rows"] * (m["in_dim"] + 3 * m["dim"]) for m in ops["mlps"])
    raw = ln.all_calls()
    ln.untouched()
    holes = [key for key, v in raw.items() if bool(torch.isnan(v).any())]
    assert not holes, f"NaN left in {holes}: an element was not written, or something outside a tensor was read and used"
    again = ln.all_calls()
    ln.untouched()
    _same(again, raw, raw.keys(), "second call")
    if variants:
        grads = [key for key in raw if key.split(".")[-1] in ("dw1", "db1", "dw2", "db2", "dwproj")]
        dins = [f"{k}.din" for k in range(ln.n)]
        ln.nan("table")                                                     # saved == NULL: the sampler's save=False
        before = ln.outs["saved"].clone()
        assert ln.fwd(save=False) == 0
        torch.cuda.synchronize()
        assert_same_bits(ln.outs["table"], raw["table"], "saved == NULL: table")
        assert torch.equal(ln.outs["saved"], before), "saved == NULL: the earlier buffer was written all the same"
        ln.nan("dbias", "scratch", *grads)                                  # dbias == NULL
        assert ln.bwd(dbias=False) == 0
        torch.cuda.synchronize()
        _same(ln.raw(), raw, grads + ["scratch"], "dbias == NULL")
        assert bool(torch.isnan(ln.outs["dbias"]).all()), "dbias == NULL: the earlier buffer was written all the same"
        for k in range(ln.n):                                               # a NULL entry of dinputs
            ln.nan(*dins)
            assert ln.din([q != k for q in range(ln.n)]) == 0
            torch.cuda.synchronize()
            _same(ln.raw(), raw, [key for q, key in enumerate(dins) if q != k], f"dinputs[{k}] == NULL")
            assert bool(torch.isnan(ln.outs[f"{k}.din"]).all())
        ln.untouched()
    return ln.unpack(raw)


# ---------------------------------------------------------------------------------------------------------------------- check A
@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_exact_relu(case):
    """Check A: operands that put every pre-activation at 0 or beyond +-16, where erff saturates and gelu_f is max(x, 0) exactly: the
    table, all of `saved`, the (dh1, dh2) rows of `scratch`, every parameter gradient, dbias and the vector dinputs have the bits of the
    int64 ReLU reference.  No tolerance anywhere."""
    ops = W.ops_a(case, R.accept_a)
    ref, info = R.ref_int(ops)
    got = run_framed(ops)
    for k in range(len(case.mlps)):
        # the precondition, on its own: a failure here is a finding about the device's erff, not about indexing
        h2, c = got[f"{k}.h2"], got[f"{k}.c"]
        assert torch.equal(c, h2.clamp(min=0)), (f"mlp {k}: gelu_f(h2) != max(h2, 0) although every |h2| is 0 or >= 16 - the device's erff "
                                                 "does not saturate at |x| >= 11.3")
    for key in ref:
        assert_same_bits(got[key], ref[key], f"{case.name} {key} (largest sum of magnitudes {info['big']})")


# ---------------------------------------------------------------------------------------------------------------------- check B
def check_b(ops, got):
    """-> ({tensor: worst err / bound}, worst embedding err / bound or None)"""
    emb_ratio = None
    for k, m in enumerate(ops["mlps"]):
        emb = got[f"{k}.emb"]
        if m["sinusoid"]:
            r = ((emb.double() - R.embed64(m["input"], m["in_dim"])).abs() / R.embed_bound(m["input"], m["in_dim"]))
            emb_ratio = max(emb_ratio or 0.0, float("inf") if bool(torch.isnan(r).any()) else r.max().item())
        else:
            assert_same_bits(emb, m["input"], f"saved input of mlp {k}")
    ref = R.ref64(ops, [got[f"{k}.emb"] for k in range(len(ops["mlps"]))])
    return R.worst_by_tensor(R.ratios(got, ref, R.bounds(ops, ref))), emb_ratio


B_TENSORS = ("table", "h1", "h2", "c", "dh2", "dh1", "dw1", "db1", "dw2", "db2", "dwproj", "dbias", "din")


def format_b(name, rat, emb, emu, emb_emu):
    line = f"  {name:<13}" + " ".join(f"{rat[key]:.3f}/{emu[key]:.3f}" for key in B_TENSORS)
    return line + ("" if emb is None else f"  emb {emb:.3f}/{emb_emu:.3f}")


@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_float64_parity(case):
    """Check B: random reals against the float64 reference under the derived bound; prints err / bound per tensor, device / emulation."""
    ops = W.ops_b(case)
    rat, emb = check_b(ops, run_framed(ops, variants=False))
    emu, emb_emu = check_b(ops, R.emulate(ops))
    print("\n" + format_b(case.name, rat, emb, emu, emb_emu))
    assert emb is None or emb <= 1.0, f"saved embedding: err / bound = {emb}"
    over = {key: r for key, r in rat.items() if not r <= 1.0}
    assert not over, f"err / bound above 1: {over}"


# ------------------------------------------------------------------------------------------------------------- library errors
def _ulp(y):
    return torch.exp2(torch.floor(torch.log2(y.abs().clamp(min=2.0 ** -126))) - 23)


def measure_erff():
    """through the (h2, c) pairs of `saved` at the device's own h2, h2 spread over [-6, 6]: (max in u |erf|, max in ulp of erf, pairs)
    over 0.5 <= |h2| <= 6, then the worst |c - gelu64(h2)| / E_gelu(h2) over all of |h2| <= 6 and the number of pairs below 0.5.
    Below 0.5 erff's own relative error cannot be told from the rounding of 1 + erf (u against K u |erf| <= 0.4 K u), so K_ERF is NOT
    measured there; what is checked there is the whole model E_gelu, which is what the bound uses."""
    g = torch.Generator().manual_seed(11)
    rows, d = 56, 256
    m = dict(sinusoid=False, in_dim=4, dim=d, input=torch.randn(rows, 4, generator=g), w1=torch.randn(d, 4, generator=g) / 2,
             b1=torch.zeros(d), w2=torch.randn(d, d, generator=g) / 16, b2=torch.rand(d, generator=g) * 12 - 6, wproj=torch.zeros(1, d))
    ln = Launch(dict(rows=rows, width=1, mlps=[m], dtable=torch.zeros(rows, 1)))
    ln.nan()
    assert ln.fwd() == 0
    torch.cuda.synchronize()
    got = ln.unpack(ln.raw())
    h2, c = got["0.h2"].double().flatten(), got["0.c"].double().flatten()
    whole = h2.abs() <= 6.0
    model = ((c - R.gelu64(h2)).abs() / R.gelu_err(h2))[whole].max().item()   # the bound's E_gelu over ALL of |h2| <= 6, small |h2| included
    small = int((h2.abs() < 0.5).sum())
    pick = (h2.abs() >= 0.5) & whole
    h2, c = h2[pick], c[pick]
    erf = torch.erf(h2 * R.RSQRT2)
    err = (c - R.gelu64(h2)).abs() * 2.0 / h2.abs()                       # all of gelu_f's error charged to erff
    return (err / (U * erf.abs())).max().item(), (err / _ulp(erf)).max().item(), int(pick.sum()), model, small


def measure_sincos():
    """through the saved embedding at i = 0, t = m 2^-14: 1000 t is exact in fp32 and f_0 = expf(0) = 1"""
    tv = torch.arange(16384, dtype=torch.float32) * 2.0 ** -14
    m = dict(sinusoid=True, in_dim=2, dim=1, input=tv, w1=torch.zeros(1, 2), b1=torch.zeros(1), w2=torch.zeros(1, 1), b2=torch.zeros(1),
             wproj=torch.zeros(1, 1))
    ln = Launch(dict(rows=16384, width=1, mlps=[m], dtable=torch.zeros(16384, 1)))
    ln.nan()
    assert ln.fwd() == 0
    torch.cuda.synchronize()
    emb = ln.unpack(ln.raw())["0.emb"].double()
    ref = R.embed64(tv, 2)
    err = (emb - ref).abs()
    return (err / (U * ref.abs().clamp(min=2.0 ** -100))).max().item(), (err / _ulp(ref)).max().item(), emb.numel()


def measure_freq():
    """relative error of the device's f_i = expf(-ln 1e4 * i / half) in u, through sin(1000 * 2^-20 * f_i): all i, half = 1..128"""
    tv = torch.tensor([2.0 ** -20])
    worst, count = 0.0, 0
    halves = list(range(1, 129))
    for q in range(0, len(halves), W.COND_MAX):
        ms = [dict(sinusoid=True, in_dim=2 * h, dim=1, input=tv, w1=torch.zeros(1, 2 * h), b1=torch.zeros(1), w2=torch.zeros(1, 1),
                   b2=torch.zeros(1), wproj=torch.zeros(1, 1)) for h in halves[q:q + W.COND_MAX]]
        ln = Launch(dict(rows=1, width=1, mlps=ms, dtable=torch.zeros(1, 1)))
        ln.nan()
        assert ln.fwd() == 0
        torch.cuda.synchronize()
        got = ln.unpack(ln.raw())
        for k, m in enumerate(ms):
            h = m["in_dim"] // 2
            s = got[f"{k}.emb"][0, :h].double()
            f = s * (1.0 + s * s / 6.0) / (1000.0 * 2.0 ** -20)              # asin(s) = s (1 + s^2 / 6 + ...), s <= 1e-3
            worst = max(worst, ((f - R.freqs64(h)).abs() / R.freqs64(h) / U).max().item())
            count += h
    return worst, count


def test_library_errors():
    """The three library errors the bound of check B cannot derive: measured on the device against float64, each at most its constant
    (4 times the value recorded in _cond_cases.py), erff / sinf / cosf at most 8 ulp of the result."""
    e_u, e_ulp, e_n, e_model, e_small = measure_erff()
    s_u, s_ulp, s_n = measure_sincos()
    f_u, f_n = measure_freq()
    print(f"\n  erff   (all of gelu_f charged to it): {e_u:.3f} u|erf| = {e_ulp:.3f} ulp over {e_n} pairs     K_ERF = {W.K_ERF}"
          f"\n  |gelu_f - gelu64| / E_gelu over all |h2| <= 6 ({e_small} pairs below 0.5, where K_ERF is assumed): {e_model:.3f}"
          f"\n  sinf / cosf, exact arguments <= 1000: {s_u:.3f} u|res| = {s_ulp:.3f} ulp over {s_n} values   K_SINCOS = {W.K_SINCOS}"
          f"\n  f = expf(-ln 1e4 i / half)          : {f_u:.3f} u relative over {f_n} (i, half)              K_FREQ = {W.K_FREQ}")
    assert e_n >= 10 ** 4 and s_n >= 10 ** 4
    assert e_ulp <= W.FINDING_ULP and s_ulp <= W.FINDING_ULP, "a finding: the device's erff / sinf / cosf errs by more than 8 ulp"
    assert e_u <= W.K_ERF and s_u <= W.K_SINCOS and f_u <= W.K_FREQ
    assert e_model <= 1.0 and e_small >= 500, "the bound's model of gelu_f's evaluation error does not hold on |x| <= 6"
    # the recorded figures stay honest: a library that moves a measured value by more than 1.5 x asks for new constants and a new table
    for got, rec, name in ((e_u, W.ERF_ERR_MEASURED, "erff"), (s_u, W.SINCOS_ERR_MEASURED, "sinf / cosf"), (f_u, W.FREQ_ERR_MEASURED, "f")):
        assert rec / 1.5 <= got <= rec * 1.5, f"{name}: measured {got:.3f}, _cond_cases.py records {rec}: re-measure and update the constants"


# ------------------------------------------------------------------------------------------------------------- vdm_cond_table_step
STEP_CASES = {"both": (3, 5, 33, True, True), "no_table_t": (3, 5, 33, False, True), "no_table_v": (3, 5, 33, True, False),
              "second_trip": (2, 5, 3301, True, True)}


@pytest.mark.parametrize("sub", STEP_CASES, ids=list(STEP_CASES))
def test_table_step(sub):
    """table[b][w] = table_t[*step][w] + table_v[b][w], bit for bit: the step from a device counter that vdm_step_inc advanced, either
    table absent, and rows * width > 64 * 256 (the grid-stride loop takes a second trip)."""
    steps, rows, width, has_t, has_v = STEP_CASES[sub]
    L = _lib().lib()
    stream = torch.cuda.current_stream().cuda_stream
    assert (rows * width > W.STEP_BLOCKS * W.THREADS) == (sub == "second_trip")
    g = torch.Generator().manual_seed(3)
    tt, tv = torch.randn(steps + 2, width, generator=g), torch.randn(rows, width, generator=g)
    bt, vt = _framed(tt)
    bv, vv = _framed(tv)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(steps):
        assert L.vdm_step_inc(counter.data_ptr(), stream) == 0
    buf, out, ok = in_sentinel(rows * width, (rows, width))
    ref = (tt[steps][None, :] if has_t else torch.zeros(1, width)) + (tv if has_v else torch.zeros(rows, width))
    for _ in range(2):
        out.fill_(NAN)
        assert L.vdm_cond_table_step(vt.data_ptr() if has_t else None, vv.data_ptr() if has_v else None,
                                     counter.data_ptr() if has_t else None, rows, width, out.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert ok() and counter.item() == steps
        assert_same_bits(out, ref, f"cond_table_step {sub}")


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refused_calls_write_nothing():
    """One refused forward (a weight matrix with 16-byte rows at a misaligned address) and one refused backward (dtable_stride <
    width): status != 0 and every output still all NaN.  The refusals themselves are tests/test_cond_cpu.py's."""
    case = W.CASES[W.CASE_IDS.index("v6_64")]
    ln = Launch(W.ops_b(case))
    ln.nan()
    ln.arr[0].w2 += 4
    assert ln.fwd() != 0 and b"aligned" in ln.L.vdm_last_error()
    ln.arr[0].w2 -= 4
    assert ln.bwd(stride=ln.width - 1) != 0 and b"bad arguments" in ln.L.vdm_last_error()
    torch.cuda.synchronize()
    ln.untouched()
    assert all(bool(torch.isnan(v).all()) for v in ln.raw().values())
