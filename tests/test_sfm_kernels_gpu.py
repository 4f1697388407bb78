"""vdm_sfm_head / vdm_sfm_loss (ABI v21) against the chain of generic launches they replace, bit for bit, and against float64.

The chain: x_t = diffuse(x1, x0, t, 1 - t) [-> diffuse(x_t, eps, 1, sigma)] -> pack_input(x_t, x0);  u = diffuse(x1, x0, 1, -1) ->
loss_terms(u, u, v_hat, u, 0) (its first sum).  Equality with it is equality of integer views: -0 and 0 differ.
Sizes: per in {4, 8, 260, 16^3 + 4, 4 * 256 * 16 * 2 + 12} - one float4 group; two groups, under a wave; ragged against the 256-voxel
round of a wave's store; 1025 groups (5 rounds of one block, 1 lane in the last); 8195 groups = 3 blocks per sample at n = 1 with a
3-group tail - at n in {1, 3}.
Bounds (u = 2^-24): x_t within 4u (|t x1| + |(1 - t) x0| + sigma |eps|) of float64 - one rounding each for 1 - t, the product, the fma
and the noise term; the sum within (per + 4) u S of float64 and d_v within 2u |d_v| - the bounds tests/test_step_kernels_gpu.py applies
to the first sum and to d_eps_hat of vdm_loss_terms_rng (_loss_random), on the target x1 - x0 rounded to fp32 as the chain rounds it."""
import pytest
import torch

from _exact import assert_same_bits, in_sentinel, ints

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16
PERS = [4, 8, 260, 16 ** 3 + 4, 4 * 256 * 16 * 2 + 12]
SHAPES = [(n, per) for n in (1, 3) for per in PERS]
CASES = [(n, per, d) for n, per in SHAPES for d in (F32, BF16)]
_sid = lambda s: f"n{s[0]}_per{s[1]}"                                                                # noqa: E731
_cid = lambda c: f"{_sid(c)}_{'f32' if c[2] == F32 else 'bf16'}"                                     # noqa: E731
WS_FLOATS = 2048 * 3
SEED, SID = (1 << 41) + 5, 3
NAN = float("nan")


def _ops():
    from vdm4cdm_amd import hip_ops
    return hip_ops


def _libmod():
    from vdm4cdm_amd import _lib
    return _lib


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def times(n, seed=9):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed))


def ibits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(got, ref, what):
    g, r = ibits(got), ibits(ref).view(got.shape)
    if not torch.equal(g, r):
        bad = (g != r).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ in their bits; first at {bad[:8].tolist()}")


def chain(ops, x0, x1, t, sigma, eps, cond, dtype):
    """(x_t, packed) of the parent's launches, in the parent's order."""
    one = torch.ones(x0.shape[0], device=DEV)
    xt = ops.diffuse(x1, x0, t.contiguous(), (1.0 - t).contiguous())
    if sigma > 0.0:
        xt = ops.diffuse(xt, eps.contiguous(), one, sigma * one)
    return xt, ops.pack_input(xt, x0 if cond else None, dtype)


def head(ops, x0, x1, t, sigma, dtype, want_x=True, **kw):
    """sfm_head into sentinel-framed outputs; asserts that nothing outside them changed."""
    n, per = x0.shape
    epl = ops.epl(dtype)
    _, packed, p_ok = in_sentinel(n * per * epl, (n, per, epl), dtype=dtype)
    _, x, x_ok = in_sentinel(n * per, (n, per))
    got_x, got_p = ops.sfm_head(x0, x1, t, sigma, dtype, x_out=x if want_x else None, packed_out=packed, **kw)
    assert got_p is packed and (got_x is x if want_x else got_x is None)
    assert p_ok() and x_ok()
    if not want_x:
        assert bool((x == -7777.0).all())
    return x, packed


# =================================================================================================== head against the chain
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_head_equals_the_chain(case):
    """x_t and both packed channels (and the zero padding) for sigma in {0, 0.1}, cond in {0, 1}, supplied and in-kernel noise."""
    ops = _ops()
    n, per, dtype = case
    x0, x1, t = rnd((n, per), 1).to(DEV), rnd((n, per), 2).to(DEV), times(n).to(DEV)
    eps_given = rnd((n, per), 3).to(DEV)
    eps_drawn = ops.randn(torch.empty((n, per), device=DEV), SEED, SID)
    for sigma in (0.0, 0.1):
        for cond in (0, 1):
            for drawn in ((False,) if sigma == 0.0 else (False, True)):
                eps = eps_drawn if drawn else eps_given
                xt_ref, p_ref = chain(ops, x0, x1, t, sigma, eps, cond, dtype)
                kw = dict(seed=SEED, stream_id=SID) if drawn else dict(eps=eps)
                x, packed = head(ops, x0, x1, t, sigma, dtype, cond=cond, **kw)
                tag = f"{_cid(case)} sigma={sigma} cond={cond} drawn={drawn}"
                same_bits(x, xt_ref, f"x_t {tag}")
                same_bits(packed, p_ref, f"packed {tag}")
                _, p2 = head(ops, x0, x1, t, sigma, dtype, want_x=False, cond=cond, **kw)            # x_t NULL: the same packed bytes
                same_bits(p2, p_ref, f"packed (x_t NULL) {tag}")


@pytest.mark.parametrize("shape", [(3, 260), (1, PERS[-1])], ids=_sid)
def test_head_draws_under_the_step_counter(shape):
    """A non-zero device step counter: the in-kernel noise is the field randn writes under that counter, not the field of counter 0."""
    ops = _ops()
    n, per = shape
    x0, x1, t = rnd((n, per), 1).to(DEV), rnd((n, per), 2).to(DEV), times(n).to(DEV)
    eps_0 = ops.randn(torch.empty((n, per), device=DEV), SEED, SID)
    counter = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    try:
        ops.SEED_STEP = counter
        eps_5 = ops.randn(torch.empty((n, per), device=DEV), SEED, SID)
        x, packed = head(ops, x0, x1, t, 0.1, F32, seed=SEED, stream_id=SID)
    finally:
        ops.SEED_STEP = None
    assert not torch.equal(eps_5, eps_0)
    xt_ref, p_ref = chain(ops, x0, x1, t, 0.1, eps_5, 1, F32)
    same_bits(x, xt_ref, f"x_t under counter 5 {shape}")
    same_bits(packed, p_ref, f"packed under counter 5 {shape}")
    assert not torch.equal(x, chain(ops, x0, x1, t, 0.1, eps_0, 1, F32)[0])


# =================================================================================================== head, exact inputs
@pytest.mark.parametrize("per", PERS)
def test_head_exact_integers(per):
    """Small integers, t in {0, 1/4, 1/2, 1} (one per sample), sigma in {0, 1/2}: every product and sum is exact - float64's values."""
    ops = _ops()
    n = 4
    t = torch.tensor([0.0, 0.25, 0.5, 1.0])
    x0, x1, eps = ints((n, per), 1, 4), ints((n, per), 2, 4), ints((n, per), 3, 4)
    for sigma in (0.0, 0.5):
        ref = (1.0 - t.double())[:, None] * x0.double() + t.double()[:, None] * x1.double() + sigma * eps.double()
        for dtype in (F32, BF16):
            x, packed = head(ops, x0.to(DEV), x1.to(DEV), t.to(DEV), sigma, dtype, eps=eps.to(DEV))
            assert_same_bits(x, ref, f"x_t integers per={per} sigma={sigma}")
            assert_same_bits(packed[..., 0].float(), ref, f"packed[0] integers per={per} sigma={sigma}")     # (multiples of 1/4 below 8: exact in bf16)
            assert_same_bits(packed[..., 1].float(), x0, f"packed[1] integers per={per}")
            assert not bool(packed[..., 2:].any())


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_head_random_against_float64(case):
    ops = _ops()
    n, per, dtype = case
    x0, x1, eps, t = rnd((n, per), 1), rnd((n, per), 2), rnd((n, per), 3), times(n)
    for sigma in (0.0, 0.1):
        s32 = float(torch.tensor(sigma, dtype=F32))                                                  # (the entry's float argument)
        a, b, c = (t.double()[:, None] * x1.double()), ((1.0 - t.double())[:, None] * x0.double()), s32 * eps.double()
        x, packed = head(ops, x0.to(DEV), x1.to(DEV), t.to(DEV), sigma, dtype, eps=eps.to(DEV))
        err, bound = (x.cpu().double() - (a + b + c)).abs(), 4 * U * (a.abs() + b.abs() + c.abs())
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        print(f"sfm_head B {_cid(case)} sigma={sigma}: max err {err.max().item():.3e}, worst err/bound {ratio:.4f}")
        assert bool((err <= bound).all()), f"sfm_head B {_cid(case)} sigma={sigma}: worst err/bound {ratio:.4f}"
        same_bits(packed[..., 0], x.to(dtype), f"packed[0] = round-to-nearest-even of x_t {_cid(case)}")
        same_bits(packed[..., 1], x0.to(DEV).to(dtype), f"packed[1] = x0 {_cid(case)}")
        assert not bool(ibits(packed[..., 2:]).any())


@pytest.mark.parametrize("shape", [(3, 260), (1, PERS[-1])], ids=_sid)
def test_head_sigma_zero_reads_no_noise(shape):
    """sigma = 0: the seed, the stream id, the step counter and a supplied (NaN) eps field change nothing."""
    ops = _ops()
    n, per = shape
    x0, x1, t = rnd((n, per), 1).to(DEV), rnd((n, per), 2).to(DEV), times(n).to(DEV)
    xa, pa = head(ops, x0, x1, t, 0.0, BF16, seed=1, stream_id=1)
    xb, pb = head(ops, x0, x1, t, 0.0, BF16, seed=(1 << 50) + 7, stream_id=2)
    xc, pc = head(ops, x0, x1, t, 0.0, BF16, eps=torch.full((n, per), NAN, device=DEV))
    for x, p, what in ((xb, pb, "another seed"), (xc, pc, "a NaN eps field")):
        same_bits(x, xa, f"x_t with {what}")
        same_bits(p, pa, f"packed with {what}")


# =================================================================================================== loss
def _ws():
    _, ws, ok = in_sentinel(WS_FLOATS, (WS_FLOATS,))
    ws.view(torch.int32).fill_(-1)
    return ws, ok


def loss(ops, vh, x0, x1, coef, pre=None):
    n, per = x0.shape
    _, sums, s_ok = in_sentinel(n, (n,))
    sums.zero_() if pre is None else sums.copy_(pre)
    _, dv, d_ok = in_sentinel(n * per, (n, per))
    ws, w_ok = _ws()
    ops.sfm_loss(vh, x0, x1, coef, sums, dv, workspace=ws)
    assert s_ok() and d_ok() and w_ok()
    return sums, dv


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_loss_equals_the_loss_terms_kernel_on_the_materialised_target(shape):
    ops = _ops()
    n, per = shape
    x0, x1, vh = rnd((n, per), 1).to(DEV), rnd((n, per), 2).to(DEV), rnd((n, per), 4).to(DEV)
    coef = (torch.rand(n, generator=torch.Generator().manual_seed(5)) + 0.1).to(DEV)
    pre = torch.arange(1, n + 1, dtype=F32, device=DEV)                                              # (sums +=: both start from the same values)
    one = torch.ones(n, device=DEV)
    u = ops.diffuse(x1, x0, one, -one)
    sums3, d_ref = torch.zeros((n, 3), device=DEV), torch.empty((n, per), device=DEV)
    sums3[:, 0] = pre
    ops.loss_terms(u, u, vh, u, 0.0, coef, sums3, d_ref)
    sums, dv = loss(ops, vh, x0, x1, coef, pre=pre)
    same_bits(sums, sums3[:, 0], f"sums {shape}")
    same_bits(dv, d_ref, f"d_v {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_loss_exact_integers(shape):
    """Integers in {-2..2}: the residual is at most 6, a sum of per squares stays below 2^24 - exact in any order; two calls accumulate."""
    ops = _ops()
    n, per = shape
    assert 2 * 36 * per + 100 < 2 ** 24
    x0, x1, vh = ints((n, per), 1, 4), ints((n, per), 2, 4), ints((n, per), 4, 4)
    coef = torch.tensor([1.0, 0.5, 2.0][:n])
    d = vh.double() - (x1.double() - x0.double())
    pre = torch.randint(0, 100, (n,), generator=torch.Generator().manual_seed(15)).float()
    sums, dv = loss(ops, vh.to(DEV), x0.to(DEV), x1.to(DEV), coef.to(DEV), pre=pre.to(DEV))
    sums2, _ = loss(ops, vh.to(DEV), x0.to(DEV), x1.to(DEV), coef.to(DEV), pre=sums)
    assert_same_bits(sums, pre.double() + (d * d).sum(1), f"sums integers {shape}")
    assert_same_bits(sums2, pre.double() + 2 * (d * d).sum(1), f"sums integers, second call {shape}")
    assert_same_bits(dv, coef.double()[:, None] * d, f"d_v integers {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_loss_random_against_float64(shape):
    ops = _ops()
    n, per = shape
    x0, x1, vh = rnd((n, per), 1), rnd((n, per), 2), rnd((n, per), 4)
    coef = torch.rand(n, generator=torch.Generator().manual_seed(5)) + 0.1
    d = vh.double() - (x1 - x0).double()                                                             # (the target as fp32 rounds it)
    S_ref, d_ref = (d * d).sum(1), coef.double()[:, None] * d
    sums, dv = loss(ops, vh.to(DEV), x0.to(DEV), x1.to(DEV), coef.to(DEV))
    for tag, err, bound in (("sums", (sums.cpu().double() - S_ref).abs(), (per + 4) * U * S_ref),
                            ("d_v", (dv.cpu().double() - d_ref).abs(), 2 * U * d_ref.abs())):
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        print(f"sfm_loss B {tag} {_sid(shape)}: max err {err.max().item():.3e}, worst err/bound {ratio:.4f}")
        assert bool((err <= bound).all()), f"sfm_loss B {tag} {_sid(shape)}: worst err/bound {ratio:.4f}"


# =================================================================================================== arguments
def _raw(name):
    L = _libmod().lib()
    return getattr(L, name), L


def test_head_refuses_bad_arguments_before_any_launch():
    """Straight through the C entry: VDM_ERR_ARG (-1) with a message naming the entry; the outputs keep their fill."""
    fn, L = _raw("vdm_sfm_head")
    n, per = 2, 260
    x0, x1, eps = (torch.zeros((n, per), device=DEV) for _ in range(3))
    t = torch.zeros(n, device=DEV)
    x = torch.full((n, per), 9.0, device=DEV)
    packed = torch.full((n, per, 4), 9.0, device=DEV)
    big = torch.zeros(n * per + 4, device=DEV)
    p = lambda a: a.data_ptr()                                                                       # noqa: E731
    good = dict(x0=p(x0), x1=p(x1), eps=p(eps), seed=1, sid=1, step=None, t=p(t), sigma=0.1, cond=1, n=n, per=per, dtype=0, x=p(x),
                packed=p(packed))
    bad = [("x0", None, "NULL"), ("x1", None, "NULL"), ("t", None, "NULL"), ("packed", None, "NULL"),
           ("per", 258, "multiple of 4"), ("per", 0, "bad sizes"), ("n", 0, "bad sizes"), ("n", -1, "bad sizes"),
           ("dtype", 7, "bad dtype"), ("sigma", -0.5, "sigma"), ("sigma", NAN, "sigma"), ("cond", 2, "cond"),
           ("x0", p(big) + 4, "16-byte aligned"), ("x1", p(big) + 4, "16-byte aligned"), ("eps", p(big) + 4, "16-byte aligned"),
           ("x", p(big) + 4, "16-byte aligned"), ("packed", p(big) + 4, "16-byte aligned"), ("t", p(big) + 2, "4-byte aligned")]
    for key, value, msg in bad:
        a = {**good, key: value}
        rc = fn(a["x0"], a["x1"], a["eps"], a["seed"], a["sid"], a["step"], a["t"], a["sigma"], a["cond"], a["n"], a["per"], a["dtype"],
                a["x"], a["packed"], torch.cuda.current_stream().cuda_stream)
        err = L.vdm_last_error().decode()
        assert rc == -1 and err.startswith("sfm_head:") and msg in err, (key, value, rc, err)
    torch.cuda.synchronize()
    assert bool((x == 9.0).all()) and bool((packed == 9.0).all())
    ops = _ops()
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.sfm_head(torch.zeros((2, 6), device=DEV), torch.zeros((2, 6), device=DEV), t, 0.0, F32)


def test_loss_refuses_bad_arguments_before_any_launch():
    fn, L = _raw("vdm_sfm_loss")
    n, per = 2, 260
    vh, x0, x1 = (torch.zeros((n, per), device=DEV) for _ in range(3))
    coef = torch.ones(n, device=DEV)
    sums = torch.full((n,), 9.0, device=DEV)
    dv = torch.full((n, per), 9.0, device=DEV)
    ws = torch.full((WS_FLOATS,), 9.0, device=DEV)
    big = torch.zeros(n * per + 4, device=DEV)
    p = lambda a: a.data_ptr()                                                                       # noqa: E731
    good = dict(vh=p(vh), x0=p(x0), x1=p(x1), coef=p(coef), n=n, per=per, sums=p(sums), dv=p(dv), ws=p(ws))
    bad = [(k, None, "NULL") for k in ("vh", "x0", "x1", "coef", "sums", "dv", "ws")] + \
          [("per", 258, "multiple of 4"), ("per", 0, "bad sizes"), ("n", 0, "bad sizes"), ("n", 2049, "at most 2048 samples"),
           ("vh", p(big) + 4, "16-byte aligned"), ("x0", p(big) + 4, "16-byte aligned"), ("x1", p(big) + 4, "16-byte aligned"),
           ("dv", p(big) + 4, "16-byte aligned"), ("coef", p(big) + 2, "4-byte aligned")]
    for key, value, msg in bad:
        a = {**good, key: value}
        rc = fn(a["vh"], a["x0"], a["x1"], a["coef"], a["n"], a["per"], a["sums"], a["dv"], a["ws"], torch.cuda.current_stream().cuda_stream)
        err = L.vdm_last_error().decode()
        assert rc == -1 and err.startswith("sfm_loss:") and msg in err, (key, value, rc, err)
    torch.cuda.synchronize()
    assert bool((sums == 9.0).all()) and bool((dv == 9.0).all()) and bool((ws == 9.0).all())
    ops = _ops()
    z = torch.zeros((2, 6), device=DEV)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.sfm_loss(z, z, z, coef, sums, torch.empty_like(z))
