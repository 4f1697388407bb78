"""The noise source and the kernels of one training / sampling step around the network (the VDM section of csrc/elementwise.hip, the
Philox code of csrc/common.h) against independent references: tests/_philox_ref.py for everything drawn, float64 / int64 formulas for
everything computed.  Shapes, windows and bounds: tests/_step_cases.py (their regimes are asserted on the CPU, tests/test_noise_cpu.py).

  N  noise source.  vdm_randn against the float64 normals of the reference on windows of a 74M-element field and on a whole second
     stream with 64-bit seed and stream id; the keying of the dropout masks and of the in-kernel time offset bit for bit (nothing
     transcendental), also under the device step counter; the three consumers that draw inside a kernel.
  A  exact integers (no tolerance): operands from _exact.ints (sparse {-1, 0, 1} where a dense sum would pass 2^24), constants powers
     of two or 1.5; outputs inside sentinels, inputs inside NaN-filled buffers, the reduce workspace exactly its documented size inside
     sentinels and filled with 0xFF bytes before every call; `sums` pre-loaded and accumulated into twice.
  B  random reals against float64 from the same fp32 inputs, u = 2^-24:
       diffuse / diffuse_pack   |dz| <= u (|alpha x| + |sigma eps| + |z|)                       (whichever way the products fuse)
       loss sums                (per + 4) u sum|terms|: the order-independent per u sum|terms| of K7b, three roundings of a term
                                (the difference or the product, its square twice) and the addition into `sums`
       d_eps_hat                2 u |coef (eh - eps)|
       ancestral_step           u (2 |ratio t| + |scale nu| + |z'|) + |ratio c sigma| |de|,  t = z - c sigma e,
                                |de| <= u (2 |(1 + w) eh| + |w eu| + |e|) under guidance, else 0
       clip_scale               8 u |c x| above the threshold (sqrt 1, add 1, divide up to 2.5, product 1, rounded up)
       elbo_assemble            4 u sum|terms|

Measured on the MI355X:
  normal transform, max |device - float64|: 1.497e-6 over the six windows of stream (42, 1) (20 544 groups; per window 1.33e-6, 1.32e-6,
  1.24e-6, 1.50e-6, 1.22e-6, 0.64e-6), 2.07e-6 over the whole second stream (2^20 groups); the bound of every noise check is 4 x the
  windows' value = 5.99e-6 (_step_cases.NORMAL_BOUND; 2^-10 = 9.8e-4 would have been a finding).  Consumers: diffuse_pack 1.2e-6,
  ancestral_step 1.1e-6, ancestral_step_rows up to 1.9e-6 (5 x 512 000).
  worst err / bound of check B, over all shapes:
    diffuse, diffuse_pack z_t     0.969   (1, 4 210 692)
    loss_terms_rng sums           0.369   (2048, 4); below 0.002 from per = 1020 on (the bound grows with per)
    loss_terms_rng d_eps_hat      0.936
    loss_terms (scalar) sums      0.371   (2048, 5)
    loss_terms (scalar) d_eps_hat 0.995   (700, 12297)
    ancestral_step                0.944 plain, 0.869 with guidance (n = 2 097 158)
    clip_scale                    0.299
    elbo_assemble                 0.232 (B = 3), 0.294 (B = 65)
"""
import functools
import math

import numpy as np
import pytest
import torch

import _philox_ref as P
import _step_cases as S
from _exact import assert_same_bits, in_sentinel, ints

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16
CONST = (1.0, 0.5, 2.0, 1.5, 0.25)                    # check A's alpha / sigma / coef: powers of two or 1.5
NAN = float("nan")


def _ops():
    from vdm4cdm_amd import hip_ops
    return hip_ops


def _libmod():
    from vdm4cdm_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- operands and framing ----------------------------------------------------------------------------------------------------------
def sparse_ints(shape, seed):
    """{-1, 0, 1} with one element in 16 non-zero: sums of squares of 2^25 of them stay near 2^21."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 32, shape, generator=g, dtype=torch.int8)
    return (r == 0).float() - (r == 1).float()


@functools.lru_cache(maxsize=6)
def field(n, per, seed):
    """Check A's operand of shape (n, per) for a kernel that sums over `per`; treat as read-only (shared among tests)."""
    if per >= 2 ** 20:
        assert (n, per) in S.VEC_SPARSE or n == 1
        return sparse_ints((n, per), seed)
    return ints((n, per), seed, terms=4 * per)        # terms up to 4^2 (a squared difference): 16 per < 2^24


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def consts(n, shift):
    return torch.tensor([CONST[(i + shift) % len(CONST)] for i in range(n)])


def nan_framed(t):
    """`t` on the device in the middle of a NaN-filled buffer: a read before or behind the operand poisons the result."""
    if t is None:
        return None
    _, v, _ = in_sentinel(t.numel(), tuple(t.shape), value=NAN, dtype=t.dtype)
    v.copy_(t)
    return v


def same(got, ref, what):
    """Bit equality with a float64 / int64 reference, decided on the device (the report of where comes from assert_same_bits)."""
    if not torch.equal(got.double(), ref.to(DEV).double().view(got.shape)):
        assert_same_bits(got, ref.view(got.shape), what)


def same_bytes(got, ref, what):
    ity = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[got.element_size()]
    g, r = got.contiguous().view(ity), ref.to(DEV).contiguous().view(ity).view(got.shape)
    if not torch.equal(g, r):
        bad = (g != r).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ in their bytes; first at {bad[:8].tolist()}")


class Workspace:
    """The reduce workspace at exactly its documented size, inside sentinels, every byte 0xFF (a NaN) before each call."""

    def __init__(self, floats):
        _, self.t, self.untouched = in_sentinel(floats, (floats,))

    def fresh(self):
        self.t.view(torch.int32).fill_(-1)
        return self.t


def spy_on(monkeypatch, *names):
    """Counts the calls of C entries that pass through the typed handle hip_ops uses."""
    L = _libmod().lib()
    calls = {n: 0 for n in names}
    for name in names:
        orig = getattr(L, name)

        def counted(*a, _orig=orig, _name=name):
            calls[_name] += 1
            return _orig(*a)
        monkeypatch.setattr(L, name, counted)
    return calls


def report(tag, err, bound):
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"{tag}: max err {err.max().item():.3e}, worst err/bound {ratio:.4f}")
    assert bool((err <= bound).all()), f"{tag}: worst err/bound {ratio:.4f}"


# =================================================================================================== N: the noise source
def _normal_err(dev_slice, ref64, tag):
    got = dev_slice.cpu().double().numpy()
    assert np.isfinite(got).all(), tag
    err = float(np.abs(got - ref64).max())
    print(f"randn {tag}: max |device - float64| {err:.3e} ({err / S.NORMAL_BOUND:.3f} of the bound {S.NORMAL_BOUND:.3e})")
    return err


def test_randn_stream_a_windows_against_float64():
    """3a.  One launch of 2048 workgroups over 18 495 200 groups (36 sweeps, the last group ragged) inside sentinels; every window of
    _step_cases.randn_windows against the reference; the zeros of the two radius-0 groups exact; the field finite and inside the
    largest radius."""
    ops = _ops()
    seed, sid = S.STREAM_A
    n = S.STREAM_A_N
    _, x, untouched = in_sentinel(n, (n,))
    ops.randn(x, seed, sid)
    assert untouched(), "vdm_randn wrote outside its n elements (the ragged last group)"
    assert bool(torch.isfinite(x).all()) and x.abs().max().item() <= S.R_MAX + S.NORMAL_BOUND
    assert not bool((x == -7777.0).any())
    worst = 0.0
    for first, count in S.randn_windows():
        lo, hi = 4 * first, min(4 * (first + count), n)
        worst = max(worst, _normal_err(x[lo:hi], P.randn(seed, sid, hi - lo, first_group=first), f"A groups {first}..{first + count}"))
    print(f"randn stream A: max over the windows {worst:.3e}")
    assert x[4 * S.G_ZERO_23 + 2].item() == 0.0 and x[4 * S.G_ZERO_23 + 3].item() == 0.0 and x[4 * S.G_ZERO_23].item() != 0.0
    assert x[4 * S.G_ZERO_01].item() == 0.0 and x[4 * S.G_ZERO_01 + 1].item() == 0.0 and x[4 * S.G_ZERO_01 + 2].item() != 0.0
    r = math.hypot(x[4 * S.G_RMAX].item(), x[4 * S.G_RMAX + 1].item())
    assert abs(r - S.R_MAX) <= 2 * S.NORMAL_BOUND, r
    assert worst <= S.NORMAL_BOUND


def test_randn_stream_b_whole_field_against_float64():
    """3a.  Seed above 2^63 and stream id above 2^40: both halves of both words reach the counter and the key."""
    ops = _ops()
    seed, sid = S.STREAM_B
    _, x, untouched = in_sentinel(S.STREAM_B_N, (S.STREAM_B_N,))
    ops.randn(x, seed, sid)
    assert untouched()
    assert _normal_err(x, P.randn(seed, sid, S.STREAM_B_N), "B whole field") <= S.NORMAL_BOUND


@pytest.mark.parametrize("step", S.SEED_STEPS[1:], ids=lambda s: f"counter{s}")
def test_randn_under_the_step_counter(step):
    """The device step counter enters the key as mix_seed(seed, counter); counter 0 gives the field of no counter, bit for bit."""
    ops = _ops()
    seed, sid, n = (1 << 40) + 5, 9, 4099
    plain = ops.randn(torch.empty(n, device=DEV), seed, sid)
    try:
        ops.SEED_STEP = torch.tensor([step], dtype=torch.int32, device=DEV)
        x = ops.randn(torch.empty(n, device=DEV), seed, sid)
    finally:
        ops.SEED_STEP = None
    assert _normal_err(x, P.randn(seed, sid, n, step=step), f"counter {step}") <= S.NORMAL_BOUND
    assert torch.equal(x, plain) == (step == 0)


def _with_counter(ops, step, fn):
    try:
        ops.SEED_STEP = None if step is None else torch.tensor([step], dtype=torch.int32, device=DEV)
        return fn()
    finally:
        ops.SEED_STEP = None


MASK_GROUPS = {32: 8, 16: 4, 96: 32, 48: 12}


@pytest.mark.parametrize("bf16,c1,c2", S.MASK_CASES, ids=[f"{'bf16' if b else 'f32'}_C{c1}+{c2}" for b, c1, c2 in S.MASK_CASES])
def test_dropout_mask_bytes_are_the_reference_bytes(bf16, c1, c2):
    """3b.  The keep byte of every 16-byte piece of a linear GroupNorm with dropout equals the reference's, for p in {0.1, 0.5}, a seed
    below and one above 2^32, without and with the device step counter (0 = the bits of no counter)."""
    ops = _ops()
    dtype = BF16 if bf16 else F32
    n, sp, C = S.MASK_N, S.MASK_SPATIAL, c1 + c2
    V = math.prod(sp)
    x1 = rnd((n,) + sp + (c1,), 31).to(DEV, dtype)
    x2 = rnd((n,) + sp + (c2,), 32).to(DEV, dtype) if c2 else None
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    st = ops.gn_stats(x1, x2, MASK_GROUPS[C])
    for p in S.MASK_PS:
        for seed in S.MASK_SEEDS:
            seen = {}
            for step in S.SEED_STEPS:
                y = _with_counter(ops, step, lambda: ops.gn_silu_fwd(x1, x2, MASK_GROUPS[C], st, gamma, beta, p, seed, want_mask=True, linear=True))
                got = y.keep_mask.cpu().numpy()
                ref = P.dropout_bytes(seed, p, n, V, C, bf16, step=step)
                assert got.shape == ref.shape and got.dtype == np.uint8
                bad = np.argwhere(got != ref)
                assert bad.size == 0, f"p={p} seed={seed} counter={step}: {len(bad)} of {ref.size} mask bytes differ, first {bad[:4].tolist()}"
                seen[step] = got
            assert np.array_equal(seen[None], seen[0]) and not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[7])


@pytest.mark.parametrize("seed", S.TIME_SEEDS, ids=lambda s: f"seed{s}")
def test_time_offset_is_the_reference_draw(seed):
    """3b.  train_scalars with neither u0 nor times: B = 1, rank 0 of 1, so t[0] is the draw itself (1.0 wraps to 0)."""
    ops = _ops()
    seen = {}
    for step in S.SEED_STEPS:
        out = _with_counter(ops, step, lambda: ops.train_scalars(1, DEV, 0, 1, -13.3, 5.0, 1.0, seed=seed))
        u = P.time_offset(seed, step)
        seen[step] = out[0, 0].item()
        assert seen[step] == (0.0 if u == 1.0 else u), (seed, step, seen[step], u)
    assert seen[None] == seen[0] and len({seen[0], seen[1], seen[7]}) == 3


def test_diffuse_pack_draws_the_batch_flat_groups():
    """3c.  x = 0, alpha = 0, sigma = 1: z_t is the drawn noise - group n * per/4 + i of the stream."""
    ops = _ops()
    c = S.PACK_NOISE
    n, per = c["n"], c["per"]
    z, packed = ops.diffuse_pack(torch.zeros((n, per), device=DEV), None, torch.zeros(n, device=DEV), torch.ones(n, device=DEV), F32,
                                 seed=c["seed"], stream_id=c["sid"], want_z=True)
    assert _normal_err(z, P.batch_noise(c["seed"], c["sid"], n, per), "diffuse_pack") <= S.NORMAL_BOUND
    assert torch.equal(packed.view(n, per, 4)[..., 0], z) and not bool(packed.view(n, per, 4)[..., 1:].any())
    assert torch.equal(z, ops.randn(torch.empty((n, per), device=DEV), c["seed"], c["sid"])), "not the field vdm_randn writes"


def _unit_table():
    """5 rows; 0 and 3 pass the noise through (ratio 1, c sigma 0, scale 1), the others are NaN: a wrong row poisons z."""
    t = torch.full((5, 4), NAN)
    t[0] = t[3] = torch.tensor([1.0, 0.0, 1.0, 0.0])
    return t.to(DEV)


@pytest.mark.parametrize("step", S.ANCESTRAL_NOISE["steps"])
def test_ancestral_step_draws_stream_step_plus_1(step):
    """3c.  z = 0, eps_hat = 0: z becomes the noise of stream id step + 1; n = 1030 ends in a ragged group."""
    ops = _ops()
    c = S.ANCESTRAL_NOISE
    n = c["n"]
    _, z, untouched = in_sentinel(n, (n,))
    z.zero_()
    ops.ancestral_step(z, torch.zeros(n, device=DEV), None, _unit_table(), torch.tensor([step], dtype=torch.int32, device=DEV), c["seed"])
    assert untouched()
    assert _normal_err(z, P.ancestral_noise(c["seed"], step, n), f"ancestral_step row {step}") <= S.NORMAL_BOUND


def _seeds_dev(seeds):
    return torch.from_numpy(np.array([int(s) & P.MASK64 for s in seeds], dtype=np.uint64).view(np.int64)).to(DEV)


@pytest.mark.parametrize("step", S.ROWS_NOISE["steps"])
def test_ancestral_rows_restart_at_group_0_of_their_seed(step):
    """3c.  Three rows; the third seed is above 2^63 and travels as its int64."""
    ops = _ops()
    c = S.ROWS_NOISE
    rows, per = len(c["seeds"]), c["per"]
    _, z, untouched = in_sentinel(rows * per, (rows, per))
    z.zero_()
    ops.ancestral_step_rows(z, torch.zeros((rows, per), device=DEV), _unit_table(), torch.tensor([step], dtype=torch.int32, device=DEV),
                            _seeds_dev(c["seeds"]))
    assert untouched()
    assert _normal_err(z, P.ancestral_rows_noise(c["seeds"], step, per), f"ancestral_step_rows row {step}") <= S.NORMAL_BOUND


@pytest.mark.parametrize("n,per", [(3, 1028), (2, 16388)])
def test_loss_terms_rng_regenerates_the_randn_fields(n, per):
    """eps / eps0 NULL: the sums and d_eps_hat of the call supplied with the vdm_randn fields of the same (seed, stream id), bit for
    bit - the batch-flat keying of diffuse_pack, pinned to the reference by the tests above."""
    ops = _ops()
    (se, ie), (s0, i0) = ((1 << 40) + 3, 1), (77, (1 << 33) + 2)
    x, eh = rnd((n, per), 41).to(DEV), rnd((n, per), 42).to(DEV)
    coef = consts(n, 1).to(DEV)
    eps, eps0 = ops.randn(torch.empty((n, per), device=DEV), se, ie), ops.randn(torch.empty((n, per), device=DEV), s0, i0)
    res = []
    for e, e0 in ((None, None), (eps, eps0), (eps, None), (None, eps0)):
        sums, deh = torch.zeros((n, 3), device=DEV), torch.empty((n, per), device=DEV)
        ops.loss_terms(x, e, eh, e0, 0.37, coef, sums, deh, rng=((se, ie), (s0, i0)))
        res.append((sums, deh))
    for sums, deh in res[1:]:
        assert torch.equal(sums, res[0][0]) and torch.equal(deh, res[0][1])


# =================================================================================================== diffuse / diffuse_pack
PLAIN_SHAPES = [(n, per) for n, per, _ in S.VEC_SHAPES] + [S.VEC_TOO_MANY]          # no workspace: 2049 samples are fine
B_SHAPES = [s for s in PLAIN_SHAPES if s != S.VEC_ONCE]
_sid = lambda s: f"n{s[0]}_per{s[1]}"                                                # noqa: E731


def _z_ref(x, eps, al, si):
    return al.double()[:, None] * x.double() + si.double()[:, None] * eps.double()


def _z_bound(x, eps, al, si):
    return U * ((al.double()[:, None] * x.double()).abs() + (si.double()[:, None] * eps.double()).abs() + _z_ref(x, eps, al, si).abs())


@pytest.mark.parametrize("shape", PLAIN_SHAPES, ids=_sid)
def test_diffuse_exact_integers(shape):
    ops = _ops()
    n, per = shape
    x, eps, al, si = field(n, per, 1), field(n, per, 2), consts(n, 0), consts(n, 2)
    _, z, untouched = in_sentinel(n * per, (n, per))
    ops.diffuse(nan_framed(x), nan_framed(eps), nan_framed(al), nan_framed(si), out=z)
    same(z, _z_ref(x, eps, al, si), f"diffuse z_t {shape}")
    assert untouched()


@pytest.mark.parametrize("shape", B_SHAPES, ids=_sid)
def test_diffuse_random_against_float64(shape):
    ops = _ops()
    n, per = shape
    x, eps, al, si = rnd((n, per), 3), rnd((n, per), 4), torch.rand(n, generator=torch.Generator().manual_seed(5)), rnd((n,), 6)
    z = ops.diffuse(nan_framed(x), nan_framed(eps), al.to(DEV), si.to(DEV))
    report(f"diffuse B {shape}", (z.cpu().double() - _z_ref(x, eps, al, si)).abs(), _z_bound(x, eps, al, si))


def _packed_ref(zref, s, dtype):
    n, per = zref.shape
    ref = torch.zeros((n, per, 4 if dtype == F32 else 8), dtype=dtype)
    ref[..., 0] = zref.to(dtype)
    if s is not None:
        ref[..., 1] = s.to(dtype)
    return ref


PACK_CASES = [(s, d) for s in PLAIN_SHAPES if s != S.VEC_ONCE for d in (F32, BF16)] + [(S.VEC_ONCE, BF16)]
_pid = lambda c: f"{_sid(c[0])}_{'f32' if c[1] == F32 else 'bf16'}"                  # noqa: E731


@pytest.mark.parametrize("case", PACK_CASES, ids=_pid)
def test_diffuse_pack_exact_integers(case):
    """z_t and every byte of the packed piece {z_t, s_cond, 0 ...} in the storage type, with and without s_cond and z_t."""
    ops = _ops()
    (n, per), dtype = case
    epl = ops.epl(dtype)
    x, eps, s, al, si = field(n, per, 1), field(n, per, 2), field(n, per, 7), consts(n, 0), consts(n, 2)
    zref = _z_ref(x, eps, al, si)
    xd, ed, sd, ald, sid_ = nan_framed(x), nan_framed(eps), nan_framed(s), nan_framed(al), nan_framed(si)
    combos = [(True, True)] if (n, per) == S.VEC_ONCE else [(a, b) for a in (True, False) for b in (True, False)]
    for with_s, with_z in combos:
        _, packed, p_ok = in_sentinel(n * per * epl, (n, per, epl), dtype=dtype)
        _, z, z_ok = in_sentinel(n * per, (n, per))
        got_z, got_p = ops.diffuse_pack(xd, sd if with_s else None, ald, sid_, dtype, eps=ed, z_out=z if with_z else None, packed_out=packed)
        assert got_p is packed and (got_z is z if with_z else got_z is None)
        same_bytes(packed, _packed_ref(zref, s if with_s else None, dtype), f"packed {case} s_cond={with_s} z_t={with_z}")
        if with_z:
            same(z, zref, f"diffuse_pack z_t {case}")
        else:
            assert bool((z == -7777.0).all())
        assert p_ok() and z_ok()


@pytest.mark.parametrize("case", [(s, d) for s in B_SHAPES for d in (F32, BF16)], ids=_pid)
def test_diffuse_pack_random_against_float64(case):
    """z_t within the bound; channel 0 of the piece is that z_t rounded to the storage type, channel 1 s_cond rounded, the rest zero -
    bit for bit."""
    ops = _ops()
    (n, per), dtype = case
    epl = ops.epl(dtype)
    x, eps, s = rnd((n, per), 3), rnd((n, per), 4), rnd((n, per), 8)
    al, si = torch.rand(n, generator=torch.Generator().manual_seed(5)), rnd((n,), 6)
    z, packed = ops.diffuse_pack(nan_framed(x), nan_framed(s), al.to(DEV), si.to(DEV), dtype, eps=nan_framed(eps), want_z=True)
    report(f"diffuse_pack B {_pid(case)}", (z.cpu().double() - _z_ref(x, eps, al, si)).abs(), _z_bound(x, eps, al, si))
    packed = packed.view(n, per, epl)
    assert torch.equal(packed[..., 0], z.view(n, per).to(dtype)) and torch.equal(packed[..., 1], s.to(DEV).to(dtype))
    assert not bool(packed[..., 2:].any())
    z2, p2 = ops.diffuse_pack(nan_framed(x), nan_framed(s), al.to(DEV), si.to(DEV), dtype, eps=nan_framed(eps), want_z=False)
    assert z2 is None and torch.equal(p2.view(n, per, epl), packed)


# =================================================================================================== loss terms
def _loss_ref(x, eps, eh, eps0, s0a0, coef):
    d = eh.double() - eps.double()
    r = float(torch.tensor(s0a0, dtype=F32)) * eps0.double()
    return torch.stack([(d * d).sum(1), (x.double() ** 2).sum(1), (r * r).sum(1)], dim=1), coef.double()[:, None] * d


def _loss_exact(ops, n, per, monkeypatch, entry):
    """Check A of either loss-terms entry through hip_ops.loss_terms (the spy names the entry the call reached)."""
    calls = spy_on(monkeypatch, "vdm_loss_terms", "vdm_loss_terms_rng")
    x, eps, eh, eps0 = (field(n, per, 10 + k) for k in range(4))
    coef, s0a0 = consts(n, 1), 0.5
    S_ref, deh_ref = _loss_ref(x, eps, eh, eps0, s0a0, coef)
    pre = torch.randint(0, 100, (n, 3), generator=torch.Generator().manual_seed(15)).double()
    want = pre + 2 * S_ref
    assert want[:, :2].max() < 2 ** 24 and 4 * want[:, 2].max() < 2 ** 24, "exact-integer check: a sum reaches 2^24"
    _, sums, s_ok = in_sentinel(n * 3, (n, 3))
    sums.copy_(pre)
    _, deh, d_ok = in_sentinel(n * per, (n, per))
    ws = Workspace(S.WS_ROWS * 3)
    xd, ed, hd, od, cd = nan_framed(x), nan_framed(eps), nan_framed(eh), nan_framed(eps0), nan_framed(coef)
    for _ in range(2):
        ops.loss_terms(xd, ed, hd, od, s0a0, cd, sums, deh, workspace=ws.fresh())
    same(sums, want, f"loss sums n={n} per={per}")
    same(deh, deh_ref, f"d_eps_hat n={n} per={per}")
    assert s_ok() and d_ok() and ws.untouched()
    assert calls == {entry: 2, ({"vdm_loss_terms", "vdm_loss_terms_rng"} - {entry}).pop(): 0}, calls


def _loss_random(ops, n, per, tag):
    x, eps, eh, eps0 = (rnd((n, per), 20 + k) for k in range(4))
    coef, s0a0 = torch.rand(n, generator=torch.Generator().manual_seed(25)) + 0.1, 0.37
    S_ref, deh_ref = _loss_ref(x, eps, eh, eps0, s0a0, coef)
    sums, deh = torch.zeros((n, 3), device=DEV), torch.empty((n, per), device=DEV)
    ops.loss_terms(nan_framed(x), nan_framed(eps), nan_framed(eh), nan_framed(eps0), s0a0, coef.to(DEV), sums, deh, workspace=Workspace(S.WS_ROWS * 3).fresh())
    report(f"{tag} B sums n={n} per={per}", (sums.cpu().double() - S_ref).abs(), (per + 4) * U * S_ref)       # every term is >= 0
    report(f"{tag} B d_eps_hat n={n} per={per}", (deh.cpu().double() - deh_ref).abs(), 2 * U * deh_ref.abs())


LOSS_RNG_SHAPES = [(n, per) for n, per, _ in S.VEC_SHAPES] + [S.LOSS_RNG_ONLY[:2]]


@pytest.mark.parametrize("shape", LOSS_RNG_SHAPES, ids=_sid)
def test_loss_terms_rng_exact_integers(shape, monkeypatch):
    _loss_exact(_ops(), *shape, monkeypatch, "vdm_loss_terms_rng")


@pytest.mark.parametrize("shape", [s for s in B_SHAPES if s != S.VEC_TOO_MANY], ids=_sid)
def test_loss_terms_rng_random_against_float64(shape):
    _loss_random(_ops(), *shape, "loss_terms_rng")


SCALAR_SHAPES = [(n, per) for n, per, _ in S.SCALAR_SHAPES]


@pytest.mark.parametrize("shape", SCALAR_SHAPES, ids=_sid)
def test_loss_terms_scalar_exact_integers(shape, monkeypatch):
    """per % 4 != 0: hip_ops.loss_terms reaches the scalar vdm_loss_terms (a cube with an odd voxel count)."""
    _loss_exact(_ops(), *shape, monkeypatch, "vdm_loss_terms")


@pytest.mark.parametrize("shape", SCALAR_SHAPES, ids=_sid)
def test_loss_terms_scalar_random_against_float64(shape):
    _loss_random(_ops(), *shape, "loss_terms")


@pytest.mark.parametrize("per", [4, 5], ids=["rng", "scalar"])
def test_loss_terms_refuse_more_samples_than_partial_rows(per):
    """2049 samples: VDM_ERR_ARG before any launch; sums and d_eps_hat keep their contents."""
    ops, lm = _ops(), _libmod()
    n = S.VEC_TOO_MANY[0]
    x, eps, eh, eps0 = (field(n, per, 10 + k).to(DEV) for k in range(4))
    _, sums, s_ok = in_sentinel(n * 3, (n, 3))
    _, deh, d_ok = in_sentinel(n * per, (n, per))
    sums.fill_(3.0)
    deh.fill_(5.0)
    ws = Workspace(S.WS_ROWS * 3)
    with pytest.raises(lm.VdmError, match="at most 2048 samples"):
        ops.loss_terms(x, eps, eh, eps0, 0.5, consts(n, 1).to(DEV), sums, deh, workspace=ws.fresh())
    torch.cuda.synchronize()
    assert bool((sums == 3.0).all()) and bool((deh == 5.0).all()) and s_ok() and d_ok()
    assert bool((ws.t.view(torch.int32) == -1).all())


# =================================================================================================== host fixes: alignment
def test_float4_entries_refuse_offset_views():
    """Views one element off 16 bytes: VdmError, nothing launched, outputs unchanged."""
    ops, lm = _ops(), _libmod()
    n, per = 2, 1028
    good = lambda: torch.zeros((n, per), device=DEV)                                   # noqa: E731
    off = lambda: torch.zeros(n * per + 4, device=DEV)[1:1 + n * per].view(n, per)     # noqa: E731
    al = torch.ones(n, device=DEV)
    z = torch.full((n, per), 9.0, device=DEV)
    zo = torch.full((n * per + 4,), 9.0, device=DEV)[1:1 + n * per].view(n, per)
    packed = torch.full((n, per, 4), 9.0, device=DEV)
    for args in ((off(), good(), z), (good(), off(), z), (good(), good(), zo)):
        with pytest.raises(lm.VdmError, match="diffuse: .*16-byte aligned"):
            ops.diffuse(args[0], args[1], al, al, out=args[2])
    for x, s, e, zz in ((off(), good(), good(), z), (good(), off(), good(), z), (good(), good(), off(), z), (good(), good(), good(), zo)):
        with pytest.raises(lm.VdmError, match="diffuse_pack: .*16-byte aligned"):
            ops.diffuse_pack(x, s, al, al, F32, eps=e, z_out=zz, packed_out=packed)
    with pytest.raises(lm.VdmError, match="diffuse_pack: .*16-byte aligned"):
        ops.diffuse_pack(good(), None, al, al, BF16, packed_out=torch.full((n * per * 8 + 8,), 9.0, device=DEV, dtype=BF16)[2:2 + n * per * 8])
    sums = torch.full((n, 3), 9.0, device=DEV)
    for x, e, h, o, d in ((off(), good(), good(), good(), z), (good(), off(), good(), good(), z), (good(), good(), off(), good(), z),
                          (good(), good(), good(), off(), z), (good(), good(), good(), good(), zo)):
        with pytest.raises(lm.VdmError, match="loss_terms_rng: .*16-byte aligned"):
            ops.loss_terms(x, e, h, o, 0.5, al, sums, d)
    torch.cuda.synchronize()
    assert bool((z == 9.0).all()) and bool((zo == 9.0).all()) and bool((packed == 9.0).all()) and bool((sums == 9.0).all())


# =================================================================================================== ancestral step
def _table():
    """5 rows of {ratio, c sigma, scale, t}: rows 0 and 3 dyadic, the others NaN."""
    t = torch.full((5, 4), NAN)
    t[0] = torch.tensor([0.5, 2.0, 1.5, 0.0])
    t[3] = torch.tensor([1.5, 0.5, 0.25, 0.0])
    return t


def _ancestral_ref(z, eh, eu, w, row, nz):
    ratio, cs, scale = (float(v) for v in row[:3])
    e = eh.double() if eu is None else (1.0 + float(torch.tensor(w, dtype=F32))) * eh.double() - float(torch.tensor(w, dtype=F32)) * eu.double()
    t = z.double() - cs * e
    return ratio * t + scale * nz.double(), t, e


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("step", S.ANCESTRAL_STEPS)
@pytest.mark.parametrize("n", S.ANCESTRAL_NS)
def test_ancestral_step_exact_integers(n, step, cfg):
    ops = _ops()
    z0, eh, eu, nz = (ints((n,), 30 + k, terms=16) for k in range(4))
    tab, w = _table(), 0.5
    ref, _, _ = _ancestral_ref(z0, eh, eu if cfg else None, w, tab[step], nz)
    _, z, untouched = in_sentinel(n, (n,))
    z.copy_(z0)
    ops.ancestral_step(z, nan_framed(eh), nan_framed(nz), nan_framed(tab), torch.tensor([step], dtype=torch.int32, device=DEV), 1,
                       eps_uncond=nan_framed(eu) if cfg else None, w_cfg=w)
    same(z, ref, f"ancestral_step n={n} row {step} cfg={cfg}")
    assert untouched()


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("n", S.ANCESTRAL_NS)
def test_ancestral_step_random_against_float64(n, cfg):
    ops = _ops()
    z0, eh, eu, nz = (rnd((n,), 40 + k) for k in range(4))
    tab, w, step = rnd((5, 4), 45), 0.3, 3
    ref, t, e = _ancestral_ref(z0, eh, eu if cfg else None, w, tab[step], nz)
    ratio, cs, scale = (float(v) for v in tab[step][:3])
    w32 = float(torch.tensor(w, dtype=F32))
    de = U * (2 * ((1 + w32) * eh.double()).abs() + (w32 * eu.double()).abs() + e.abs()) if cfg else torch.zeros(n, dtype=torch.float64)
    bound = U * (2 * (ratio * t).abs() + (scale * nz.double()).abs() + ref.abs()) + abs(ratio * cs) * de
    z = z0.to(DEV)
    ops.ancestral_step(z, eh.to(DEV), nz.to(DEV), tab.to(DEV), torch.tensor([step], dtype=torch.int32, device=DEV), 1,
                       eps_uncond=eu.to(DEV) if cfg else None, w_cfg=w)
    report(f"ancestral_step B n={n} cfg={cfg}", (z.cpu().double() - ref).abs(), bound)


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("step", S.ANCESTRAL_STEPS)
@pytest.mark.parametrize("n", S.ANCESTRAL_NS)
def test_ancestral_step_drawn_noise_is_the_randn_field(n, step, cfg):
    """noise NULL: the bits of the call supplied with the field vdm_randn writes for (seed, step + 1)."""
    ops = _ops()
    seed = (1 << 40) + 17
    z0, eh, eu = (rnd((n,), 50 + k).to(DEV) for k in range(3))
    tab, sp = rnd((5, 4), 55).to(DEV), torch.tensor([step], dtype=torch.int32, device=DEV)
    noise = ops.randn(torch.empty(n, device=DEV), seed, step + 1)
    za, zb = z0.clone(), z0.clone()
    ops.ancestral_step(za, eh, None, tab, sp, seed, eps_uncond=eu if cfg else None, w_cfg=0.3)
    ops.ancestral_step(zb, eh, noise, tab, sp, seed, eps_uncond=eu if cfg else None, w_cfg=0.3)
    assert torch.equal(za, zb) and not torch.equal(za, z0)


def _row_seeds(rows):
    """One seed per row over all of 64 bits (row r: r * the golden ratio mod 2^64, row 0 bumped to 1)."""
    s = (np.arange(rows, dtype=np.uint64) * np.uint64(P.GOLDEN64)) + np.uint64(1)
    return s, torch.from_numpy(s.view(np.int64)).to(DEV)


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("shape", S.ROWS_SHAPES, ids=lambda s: f"rows{s[0]}_per{s[1]}")
def test_ancestral_rows_update_exact_integers(shape, cfg):
    """scale = 0 removes the (finite) noise: the deterministic part of the row-keyed update, exact."""
    ops = _ops()
    rows, per = shape
    z0, eh, eu = (ints((rows, per), 60 + k, terms=16) for k in range(3))
    tab, w, step = _table(), 0.5, 3
    tab[step, 2] = 0.0
    ref, _, _ = _ancestral_ref(z0, eh, eu if cfg else None, w, tab[step], torch.zeros(rows, per))
    _, z, untouched = in_sentinel(rows * per, (rows, per))
    z.copy_(z0)
    ops.ancestral_step_rows(z, nan_framed(eh), nan_framed(tab), torch.tensor([step], dtype=torch.int32, device=DEV), _row_seeds(rows)[1],
                            eps_uncond=nan_framed(eu) if cfg else None, w_cfg=w)
    same(z, ref, f"ancestral_step_rows {shape} cfg={cfg}")
    assert untouched()


@pytest.mark.parametrize("shape", S.ROWS_SHAPES, ids=lambda s: f"rows{s[0]}_per{s[1]}")
def test_ancestral_rows_noise_at_every_grid(shape):
    """z = 0, eps_hat = 0, unit row: every row is the reference field of its own seed, at every grid shape (one workgroup per row up to
    the capped 410 per row)."""
    ops = _ops()
    rows, per = shape
    step = 3
    seeds, seeds_dev = _row_seeds(rows)
    _, z, untouched = in_sentinel(rows * per, (rows, per))
    z.zero_()
    ops.ancestral_step_rows(z, torch.zeros((rows, per), device=DEV), _unit_table(), torch.tensor([step], dtype=torch.int32, device=DEV), seeds_dev)
    assert untouched()
    assert _normal_err(z, P.ancestral_rows_noise(seeds, step, per), f"ancestral_step_rows {shape}") <= S.NORMAL_BOUND


def test_ancestral_rows_refuses_65536_rows():
    ops, lm = _ops(), _libmod()
    rows = S.ROWS_REFUSED
    z = torch.full((rows, 4), 9.0, device=DEV)
    with pytest.raises(lm.VdmError, match="rows = 65536"):
        ops.ancestral_step_rows(z, torch.zeros((rows, 4), device=DEV), _unit_table(), torch.zeros(1, dtype=torch.int32, device=DEV), _row_seeds(rows)[1])
    torch.cuda.synchronize()
    assert bool((z == 9.0).all())


# =================================================================================================== sumsq / clip_scale
@pytest.mark.parametrize("n", S.SUMSQ_NS)
def test_sumsq_exact_integers(n):
    """Accumulates into a pre-loaded out; its own workspace of exactly 2048 floats."""
    ops = _ops()
    x = field(1, n, 70).view(n)
    want = 5.0 + 2 * (x.double() ** 2).sum()
    assert want < 2 ** 24
    _, out, o_ok = in_sentinel(1, (1,))
    out.fill_(5.0)
    ws = Workspace(2048)
    xd = nan_framed(x)
    for _ in range(2):
        ops.sumsq(xd, out, workspace=ws.fresh())
    assert out.item() == want.item(), (out.item(), want.item())
    assert o_ok() and ws.untouched()


def test_sumsq_refuses_an_offset_pointer():
    ops, lm = _ops(), _libmod()
    out = torch.full((1,), 5.0, device=DEV)
    with pytest.raises(lm.VdmError, match="sumsq: x must be 16-byte aligned"):
        ops.sumsq(torch.ones(1028, device=DEV)[1:], out)
    torch.cuda.synchronize()
    assert out.item() == 5.0


@pytest.mark.parametrize("n", S.CLIP_NS)
def test_clip_scale_below_and_above_the_threshold(n):
    ops = _ops()
    x0 = rnd((n,), 71)
    special = torch.from_numpy(np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x80000000, 1, 0x007FFFFF, 0x807FFFFF, 0x7F800000],
                                        dtype=np.uint32).view(np.int32))           # NaN patterns, -0, denormals, inf
    k = min(n, special.numel())
    x0.view(torch.int32)[:k] = special[:k]
    _, x, untouched = in_sentinel(n, (n,))
    x.copy_(x0)
    ops.clip_scale_(x, torch.tensor([0.25], device=DEV), 1.0)              # norm 0.5 < max_norm 1: coefficient 1
    assert torch.equal(x.view(torch.int32).cpu(), x0.view(torch.int32)), "below the threshold x must keep its bits"
    x1 = rnd((n,), 72)
    x.copy_(x1)
    sumsq, max_norm = torch.tensor([7.3]), 0.9
    c = max_norm / (math.sqrt(float(sumsq[0])) + 1.0e-6)
    ops.clip_scale_(x, sumsq.to(DEV), max_norm)
    ref = c * x1.double()
    report(f"clip_scale B n={n}", (x.cpu().double() - ref).abs(), 8 * U * ref.abs())
    assert untouched()


# =================================================================================================== elbo_assemble / pack_input
def _elbo(ops, sums, coef, k):
    lm = _libmod()
    _, out, untouched = in_sentinel(4, (4,))
    sums_d, coef_d = nan_framed(sums), nan_framed(coef)                    # (named: the buffers must outlive the launch)
    lm.check(lm.lib().vdm_elbo_assemble(sums_d.data_ptr(), coef_d.data_ptr(), sums.shape[0], *k, out.data_ptr(), _stream()), "vdm_elbo_assemble")
    torch.cuda.synchronize()
    assert untouched()
    return out.cpu().double()


def _elbo_terms(sums, coef, k):
    k = [float(torch.tensor(v, dtype=F32)) for v in k]
    s, B = sums.double(), sums.shape[0]
    diff, lat, rec = 0.5 * coef.double() * s[:, 0], k[0] + k[1] * s[:, 1], k[2] * s[:, 2] + k[3]
    ref = torch.stack([diff.sum() + lat.sum() / B + rec.sum() / B, diff.sum(), lat.sum() / B, rec.sum() / B])
    a = [diff.abs().sum(), (abs(k[0]) + (k[1] * s[:, 1]).abs()).sum() / B, ((k[2] * s[:, 2]).abs() + abs(k[3])).sum() / B]
    return ref, torch.stack([a[0] + a[1] + a[2], a[0], a[1], a[2]])


@pytest.mark.parametrize("B", S.ELBO_EXACT_B)
def test_elbo_assemble_exact(B):
    """Integer sums in 0..7, dyadic coefficients and constants, B a power of two: every partial sum has fewer than 24 bits."""
    sums = torch.randint(0, 8, (B, 3), generator=torch.Generator().manual_seed(80)).float()
    k = (0.5, 0.25, 1.5, -2.0)
    ref, mag = _elbo_terms(sums, consts(B, 0), k)
    assert mag.max() * 16 < 2 ** 24 and B & (B - 1) == 0
    got = _elbo(_ops(), sums, consts(B, 0), k)
    assert torch.equal(got, ref), (got, ref)


@pytest.mark.parametrize("B", S.ELBO_REAL_B)
def test_elbo_assemble_random_against_float64(B):
    sums, coef, k = rnd((B, 3), 81), rnd((B,), 82), (0.31, -0.27, 1.7, -0.9)
    ref, mag = _elbo_terms(sums, coef, k)
    report(f"elbo_assemble B B={B}", (_elbo(_ops(), sums, coef, k) - ref).abs(), 4 * U * mag)


@pytest.mark.parametrize("with_b", [True, False], ids=["b", "b_null"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("nvox", S.PACK_INPUT_NVOX)
def test_pack_input_every_byte(nvox, dtype, with_b):
    ops = _ops()
    cp = ops.cpad(2, dtype)
    a, b = rnd((nvox,), 90), (rnd((nvox,), 91) if with_b else None)
    ref = torch.zeros((nvox, cp), dtype=dtype)
    ref[:, 0] = a.to(dtype)
    if with_b:
        ref[:, 1] = b.to(dtype)
    _, out, untouched = in_sentinel(nvox * cp, (nvox, cp), dtype=dtype)
    ops.pack_input(nan_framed(a), nan_framed(b), dtype, out=out)
    same_bytes(out, ref, f"pack_input nvox={nvox}")
    assert untouched()
