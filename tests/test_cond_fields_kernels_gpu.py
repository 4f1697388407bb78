"""Kernel-level tests of the entries behind several conditioning fields (CUNet(s_conditioning_channels = K), K in 1..3), each alone
through its hip_ops wrapper: vdm_pack_fields, vdm_diffuse_pack_fields, vdm_conv_in_dgrad_fields, and conv_in itself (forward and weight
gradient of the generic conv kernels at cin = 3, 4).

The checkers are never the code under test: pack_input (a separate kernel), float64 torch on the CPU (exact-integer check A, random-
data check B with the bound of tests/test_input_grad_kernels_gpu.py) and sentinel buffers around the outputs.  The single-field entries
diffuse_pack and conv_in_dgrad launch the kernels of the _fields entries (one head kernel, one K1t kernel): bit equality with them says
that the two entries hand the kernel the same arguments; at K = 1 and cin <= 2 both sides run the same instantiation, which is not an
independent check - those come from test_diffuse_pack_fields_exact_integers and the float64 K1t checks of
tests/test_input_grad_kernels_gpu.py.
"""
import pytest
import torch
import torch.nn.functional as F

from _exact import assert_same_bits, in_sentinel, ints

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U32 = 2.0 ** -24                      # unit roundoff of fp32
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
# one thread group; under one wave; ragged against the 256-voxel wave round; several blocks (16 * 256 groups per block) + a tail
PERS = [4, 8, 260, 16 * 16 * 16 + 4, 4 * 256 * 16 * 2 + 12]


def _mods():
    from vdm4cdm_amd import _lib
    from vdm4cdm_amd import hip_ops
    return _lib, hip_ops


def rnd(shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * scale
    return x.to(dtype).float()


def _bits(t):
    """The storage bits of a tensor as integers (bf16 -> int16, fp32 -> int32): equality that tells -0 from 0 and compares NaNs."""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# =============================================================================================== vdm_pack_fields
@pytest.mark.parametrize("per", PERS, ids=[f"per{p}" for p in PERS])
@pytest.mark.parametrize("n", [1, 3], ids=["n1", "n3"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", [1, 2, 3], ids=["k1", "k2", "k3"])
def test_pack_fields_equals_pack_input_per_channel(k, dtype, n, per):
    """Channel 0 and channel 1 + j are, bit for bit, channels 0 and 1 of pack_input(z, c_j); every other channel is exactly +0; the
    output sits inside a sentinel buffer that stays untouched outside."""
    _lib, ops = _mods()
    z, cond = rnd((n, per), 1).to(DEV), rnd((n, k, per), 2).to(DEV)
    cp = ops.cpad(1 + k, dtype)
    assert cp * (2 if dtype == torch.bfloat16 else 4) == 16, "one 16-byte piece per voxel"
    buf, view, untouched = in_sentinel(n * per * 4, (n, per, 4))            # 16 bytes per voxel in either storage type
    out = view.view(dtype).view(n, per, cp) if dtype == torch.bfloat16 else view
    got = ops.pack_fields(z, cond, dtype, out=out)
    torch.cuda.synchronize()
    assert untouched(), "pack_fields wrote outside its output"
    assert got.shape == (n, per, cp) and got.dtype == dtype
    for j in range(k):
        ref = ops.pack_input(z, cond[:, j].contiguous(), dtype)
        assert torch.equal(_bits(got[..., 0]), _bits(ref[..., 0])), f"channel 0 (z) differs from pack_input (field {j})"
        assert torch.equal(_bits(got[..., 1 + j]), _bits(ref[..., 1])), f"channel {1 + j} differs from pack_input's channel 1"
    assert bool((_bits(got[..., 1 + k:]) == 0).all()), "padding channels are not +0"


def test_pack_fields_refuses_a_voxel_count_that_is_no_multiple_of_4():
    """The kernel owns 4 voxels per thread: hip_ops refuses (ValueError) instead of falling back, and the entry returns VDM_ERR_ARG."""
    _lib, ops = _mods()
    z, cond = torch.zeros(1, 6, device=DEV), torch.zeros(1, 2, 6, device=DEV)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.pack_fields(z, cond, torch.float32)
    out = torch.zeros(1, 6, 4, device=DEV)
    L = _lib.lib()
    assert L.vdm_pack_fields(z.data_ptr(), cond.data_ptr(), 2, 1, 6, 0, out.data_ptr(), None) == -1 and b"multiple of 4" in L.vdm_last_error()


# =============================================================================================== vdm_diffuse_pack_fields
def _head_inputs(n, k, per, seed):
    x, cond, eps = rnd((n, 1, per, 1, 1), seed).to(DEV), rnd((n, k, per, 1, 1), seed + 1).to(DEV), rnd((n, 1, per, 1, 1), seed + 2).to(DEV)
    g = torch.Generator().manual_seed(seed + 3)
    gam = (torch.rand(n, generator=g) * 20 - 10)
    return x, cond, eps, torch.sqrt(torch.sigmoid(-gam)).to(DEV), torch.sqrt(torch.sigmoid(gam)).to(DEV)


@pytest.mark.parametrize("per", PERS, ids=[f"per{p}" for p in PERS])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", [1, 2, 3], ids=["k1", "k2", "k3"])
@pytest.mark.parametrize("noise", ["supplied", "in_kernel"])
def test_diffuse_pack_fields_equals_diffuse_pack(noise, k, dtype, per):
    """z_t, packed channel 0 and channel 1 equal diffuse_pack(x, c_0, ...) bit for bit (the same Philox counters, the same rounding);
    channels 2.. equal pack_fields; with z_t = None the packed output does not change.  Both entries launch the one head kernel: at
    k1 the two sides run the same instantiation (the entries' argument mapping is what is compared), at k2 / k3 sibling instantiations;
    the independent reference is test_diffuse_pack_fields_exact_integers."""
    _lib, ops = _mods()
    n = 3 if per < 1000 else 2
    x, cond, eps, al, si = _head_inputs(n, k, per, 10 * k + per % 97)
    kw = dict(eps=eps) if noise == "supplied" else dict(seed=(1 << 40) + 12345, stream_id=5)
    z, packed = ops.diffuse_pack_fields(x, cond, al, si, dtype, want_z=True, **kw)
    z1, packed1 = ops.diffuse_pack(x, cond[:, :1].contiguous(), al, si, dtype, want_z=True, **kw)
    assert z.shape == x.shape and packed.shape == packed1.shape == (n, per, 1, 1, ops.cpad(1 + k, dtype))
    assert torch.equal(_bits(z), _bits(z1)), "z_t differs from vdm_diffuse_pack"
    assert torch.equal(_bits(packed[..., :2]), _bits(packed1[..., :2])), "packed channels 0 / 1 differ from vdm_diffuse_pack"
    plain = ops.pack_fields(z.view(n, per), cond.view(n, k, per), dtype).view(packed.shape)
    assert torch.equal(_bits(packed[..., 2:]), _bits(plain[..., 2:])), "channels 2.. differ from vdm_pack_fields"
    none, packed0 = ops.diffuse_pack_fields(x, cond, al, si, dtype, want_z=False, **kw)
    assert none is None and torch.equal(_bits(packed0), _bits(packed))


HEAD_CONST = (1.0, 0.5, 2.0, 1.5, 0.25)               # alpha / sigma of the exact check: powers of two or 1.5
HEAD_A_SHAPES = [(3, 4), (3, 260), (2, 16 * 16 * 16 + 4)]      # one lane; ragged against the 256-voxel round; several rounds + a one-lane tail


def _nan_framed(t):
    """`t` on the device in the middle of a NaN-filled buffer: a read before or behind the operand poisons the result."""
    _, v, _ = in_sentinel(t.numel(), tuple(t.shape), value=float("nan"))
    v.copy_(t)
    return v


@pytest.mark.parametrize("shape", HEAD_A_SHAPES, ids=[f"n{n}_per{p}" for n, p in HEAD_A_SHAPES])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k", [2, 3], ids=["k2", "k3"])
def test_diffuse_pack_fields_exact_integers(k, dtype, shape):
    """A reference that is no sibling instantiation of the head kernel: x, eps and the K planes uniform in {-2..2}, alpha and sigma in
    {1, 0.5, 2, 1.5, 0.25}, so alpha x + sigma eps is a multiple of 1/4 of magnitude <= 8 - exact in fp32 in any order and rounding,
    and exact in bf16 (6 significant bits at the most).  z_t must have the bits of the float64 expression and every byte of the piece
    {z_t, c_0 .. c_{K-1}, 0 ...} those of the reference in the storage type, with and without z_t; the inputs sit in NaN frames, the
    outputs inside sentinels (the C entry directly: the wrapper allocates its outputs)."""
    _lib, ops = _mods()
    n, per = shape
    epl = ops.cpad(1 + k, dtype)
    x, eps, cond = ints((n, per), 31, terms=4), ints((n, per), 32, terms=4), ints((n, k, per), 33, terms=4)
    al = torch.tensor([HEAD_CONST[i % 5] for i in range(n)])
    si = torch.tensor([HEAD_CONST[(i + 2) % 5] for i in range(n)])
    zref = al.double()[:, None] * x.double() + si.double()[:, None] * eps.double()
    assert zref.abs().max() <= 8 and torch.equal(zref * 4, (zref * 4).round())
    ref = torch.zeros((n, per, epl), dtype=dtype)
    ref[..., 0] = zref.to(dtype)
    ref[..., 1:1 + k] = cond.permute(0, 2, 1).to(dtype)
    assert torch.equal(ref[..., 0].double(), zref), "the storage type does not hold z_t exactly"
    ity = torch.int16 if dtype == torch.bfloat16 else torch.int32
    xd, ed, cd, ald, sid = _nan_framed(x), _nan_framed(eps), _nan_framed(cond), _nan_framed(al), _nan_framed(si)
    for with_z in (True, False):
        _, packed, p_ok = in_sentinel(n * per * epl, (n, per, epl), dtype=dtype)
        z_buf, z, z_ok = in_sentinel(n * per, (n, per))
        _lib.check(_lib.lib().vdm_diffuse_pack_fields(xd.data_ptr(), cd.data_ptr(), k, ed.data_ptr(), 0, 0, None, ald.data_ptr(), sid.data_ptr(), n,
                                                      per, ops.dt_id(dtype), z.data_ptr() if with_z else None, packed.data_ptr(), None),
                   "vdm_diffuse_pack_fields")
        torch.cuda.synchronize()
        assert p_ok() and z_ok(), "diffuse_pack_fields wrote outside packed / z_t"
        bad = (packed.view(ity) != ref.to(DEV).view(ity)).nonzero()
        assert bad.shape[0] == 0, f"packed z_t={with_z}: {bad.shape[0]} elements differ in their bytes; first at {bad[:8].tolist()}"
        if with_z:
            assert_same_bits(z, zref, "diffuse_pack_fields z_t")
        else:
            assert bool((z_buf == -7777.0).all()), "z_t was written without being asked for"


def test_diffuse_pack_fields_with_a_seed_step_counter():
    """The graph-captured training step keys its noise by a device counter (hip_ops.SEED_STEP): with a non-zero counter the entry still
    draws the field vdm_diffuse_pack draws, and another field than with the counter at zero."""
    _lib, ops = _mods()
    n, k, per = 2, 2, 260
    x, cond, _, al, si = _head_inputs(n, k, per, 77)
    prev = ops.SEED_STEP
    try:
        ops.SEED_STEP = torch.tensor([5], dtype=torch.int32, device=DEV)
        z, packed = ops.diffuse_pack_fields(x, cond, al, si, torch.bfloat16, seed=99, stream_id=1, want_z=True)
        z1, packed1 = ops.diffuse_pack(x, cond[:, :1].contiguous(), al, si, torch.bfloat16, seed=99, stream_id=1, want_z=True)
        ops.SEED_STEP = torch.tensor([0], dtype=torch.int32, device=DEV)
        z0, _ = ops.diffuse_pack_fields(x, cond, al, si, torch.bfloat16, seed=99, stream_id=1, want_z=True)
        torch.cuda.synchronize()
    finally:
        ops.SEED_STEP = prev
    assert torch.equal(_bits(z), _bits(z1)) and torch.equal(_bits(packed[..., :2]), _bits(packed1[..., :2]))
    assert not torch.equal(z, z0), "the step counter does not reach the noise key"


# =============================================================================================== vdm_conv_in_dgrad_fields (K1t)
def ref_conv_in_dgrad(dh, weight, cin, circular, dtype=torch.float64):
    """dh [N, D, H, W, C], weight [27, C, cin] -> the gradient of conv_in's input [N, cin, D, H, W]: autograd of F.conv3d at a zero
    input in float64 (restated from tests/test_input_grad_kernels_gpu.py)."""
    n, d, h, w, c = dh.shape
    x = torch.zeros(n, cin, d, h, w, dtype=dtype, requires_grad=True)
    wt = weight.to(dtype).view(3, 3, 3, c, cin).permute(3, 4, 0, 1, 2)
    y = F.conv3d(F.pad(x, (1,) * 6, mode="circular"), wt) if circular else F.conv3d(x, wt, padding=1)
    y.backward(dh.to(dtype).permute(0, 4, 1, 2, 3))
    return x.grad


K1T_RAGGED = [(5, 7, 18), (6, 9, 20)]
K1T_TINY = [(1, 1, 1), (2, 2, 2), (1, 5, 3)]
K1T_OTHER = [(4, 4, 16), (3, 4, 33), (17, 3, 16)]


def _k1t_cases():
    """Every (C, cin, storage, padding) combination gets one grid of each family; grids and batch size rotate as in
    tests/test_input_grad_kernels_gpu.py."""
    cases, i = [], 0
    for C in (16, 32, 48, 64):
        for cin in (3, 4):
            for dtype in DTYPES:
                for circular in (False, True):
                    r = i // 2 + (i % 2) * 5
                    grids = [(K1T_RAGGED[r % 2], 3 if (r // 2) % 2 == 0 else 1), (K1T_TINY[r % 3], 1 if r % 2 == 0 else 3),
                             (K1T_OTHER[(r + i // 8) % 3], 1 if (r // 4) % 2 == 0 else 3)]
                    for grid, n in grids:
                        cases.append((C, cin, dtype, circular, grid, n))
                    i += 1
    return cases


def _k1t_id(c):
    C, cin, dtype, circular, (d, h, w), n = c
    return f"C{C}_cin{cin}_{'f32' if dtype == torch.float32 else 'bf16'}_{'circ' if circular else 'zeros'}_{d}x{h}x{w}_N{n}"


K1T_CASES = _k1t_cases()


def test_k1t_fields_case_table():
    combos = {}
    for C, cin, dtype, circular, grid, n in K1T_CASES:
        combos.setdefault((C, cin, dtype, circular), []).append((grid, n))
    assert len(combos) == 32
    for key, gs in combos.items():
        assert any(g in K1T_RAGGED for g, _ in gs) and any(g in K1T_TINY for g, _ in gs) and any(g in K1T_OTHER for g, _ in gs), key
    for grid in K1T_RAGGED + K1T_TINY + K1T_OTHER:
        seen = [(dtype, circular, cin) for _, cin, dtype, circular, g, n in K1T_CASES if g == grid]
        assert {s[0] for s in seen} == set(DTYPES) and {s[1] for s in seen} == {False, True} and {s[2] for s in seen} == {3, 4}, grid
    assert {n for *_, n in K1T_CASES} == {1, 3}


def _k1t_run(dh, weight, cin, dtype, circular, want_s=True):
    _lib, ops = _mods()
    n, d, h, w, _ = dh.shape
    dz, ds = ops.conv_in_dgrad_fields(dh.to(dtype).to(DEV).contiguous(), weight.to(DEV), cin, circular, want_s=want_s)
    assert dz.dtype == torch.float32 and dz.shape == (n, d, h, w)
    if not want_s or cin == 1:
        assert ds is None
        return dz.cpu()[:, None]
    assert ds.shape == (n, cin - 1, d, h, w)
    return torch.cat([dz[:, None], ds], dim=1).cpu()          # [N, cin, D, H, W] like the reference


@pytest.mark.parametrize("case", K1T_CASES, ids=_k1t_id)
def test_k1t_fields_exact_integers(case):
    """Check A: dh and W uniform in {-2..2}: every partial sum is an integer of magnitude <= 4 * 27 * C, the kernel must give the bits
    of the float64 transposed convolution - and dz alone (n_ds = 0) the bits of the full call."""
    C, cin, dtype, circular, (d, h, w), n = case
    dh, wt = ints((n, d, h, w, C), 11, terms=27 * C), ints((27, C, cin), 12, terms=27 * C)
    got = _k1t_run(dh, wt, cin, dtype, circular)
    assert_same_bits(got, ref_conv_in_dgrad(dh, wt, cin, circular), _k1t_id(case))
    assert torch.equal(_k1t_run(dh, wt, cin, dtype, circular, want_s=False), got[:, :1]), "dz depends on n_ds"


@pytest.mark.parametrize("case", K1T_CASES, ids=_k1t_id)
def test_k1t_fields_random_against_float64(case):
    """Check B, per output voxel q: |got - ref64| <= (27 C + 1) 2^-24 S(q), S = the same transposed convolution of |dh| and |W| (the
    running-error bound of an fp32 dot product of 27 C terms in any order; the bound of tests/test_input_grad_kernels_gpu.py)."""
    C, cin, dtype, circular, (d, h, w), n = case
    dh, wt = rnd((n, d, h, w, C), 21, dtype), rnd((27, C, cin), 22, scale=0.2)
    got = _k1t_run(dh, wt, cin, dtype, circular).double()
    ref = ref_conv_in_dgrad(dh, wt, cin, circular)
    bound = (27 * C + 1) * U32 * ref_conv_in_dgrad(dh.abs(), wt.abs(), cin, circular)
    err = (got - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"K1t fields B {_k1t_id(case)}: max err {err.max().item():.3e}, worst err/bound {worst:.4f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), f"worst err / bound {worst}"
    dz0 = _k1t_run(dh, wt, cin, dtype, circular, want_s=False)
    assert torch.equal(dz0.double(), got[:, :1]), "dz depends on n_ds"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("circular", [False, True], ids=["zeros", "circ"])
@pytest.mark.parametrize("cin", [1, 2])
def test_k1t_fields_equals_the_single_field_entry(cin, circular, dtype):
    """cin in {1, 2}: the bits of vdm_conv_in_dgrad on random data.  Both entries launch the same instantiation of the one K1t kernel,
    so this compares their argument mapping (ds [n][1][vol] = [n][vol]); vdm_conv_in_dgrad's independent reference is float64
    (tests/test_input_grad_kernels_gpu.py)."""
    _lib, ops = _mods()
    for k, (n, grid, C) in enumerate([(3, (5, 7, 18), 48), (1, (1, 5, 3), 16), (2, (3, 4, 33), 64)]):
        dh = rnd((n,) + grid + (C,), 40 + k, dtype).to(dtype).to(DEV)
        wt = rnd((27, C, cin), 50 + k, scale=0.2).to(DEV)
        dz, ds = ops.conv_in_dgrad_fields(dh, wt, cin, circular, want_s=True)
        dz1, ds1 = ops.conv_in_dgrad(dh, wt, cin, circular, want_s=(cin == 2))
        assert torch.equal(_bits(dz), _bits(dz1))
        assert (ds is None and ds1 is None) or torch.equal(_bits(ds[:, 0]), _bits(ds1))


@pytest.mark.parametrize("cin,n_ds", [(3, 2), (4, 0), (4, 3)], ids=["cin3_ds", "cin4_dz_only", "cin4_ds"])
def test_k1t_fields_writes_inside_its_outputs(cin, n_ds):
    """dz and ds as slices of sentinel-filled buffers (the C entry directly): nothing outside is written, with n_ds = 0 ds is not
    touched at all."""
    _lib, ops = _mods()
    n, (d, h, w), C = 2, (5, 7, 18), 32
    dh, wt = ints((n, d, h, w, C), 61, terms=27 * C), ints((27, C, cin), 62, terms=27 * C)
    dh_d, wt_d = dh.to(torch.bfloat16).to(DEV).contiguous(), wt.to(DEV)
    _, dz, dz_ok = in_sentinel(n * d * h * w, (n, d, h, w))
    ds_buf, ds, ds_ok = in_sentinel(n * (cin - 1) * d * h * w, (n, cin - 1, d, h, w))
    _lib.check(_lib.lib().vdm_conv_in_dgrad_fields(dh_d.data_ptr(), n, d, h, w, C, _lib.VDM_BF16, _lib.PAD_ZEROS, wt_d.data_ptr(), cin, dz.data_ptr(),
                                                   ds.data_ptr() if n_ds else None, n_ds, None), "vdm_conv_in_dgrad_fields")
    torch.cuda.synchronize()
    assert dz_ok() and ds_ok(), "conv_in_dgrad_fields wrote outside dz / ds"
    ref = ref_conv_in_dgrad(dh, wt, cin, False)
    assert_same_bits(dz.cpu(), ref[:, 0], "dz inside the sentinel buffer")
    if n_ds:
        assert_same_bits(ds.cpu(), ref[:, 1:], "ds inside the sentinel buffer")
    else:
        assert bool((ds_buf == -7777.0).all()), "ds was written with n_ds = 0"


# =============================================================================================== conv_in as a conv at cin = 3, 4
def _padded_dev(t, dtype, cp):
    out = torch.zeros(t.shape[:-1] + (cp,), dtype=dtype, device=DEV)
    out[..., :t.shape[-1]] = t.to(dtype).to(DEV)
    return out


def _small_ints(shape, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8).float()


@pytest.mark.parametrize("n,grid", [(1, (5, 7, 18)), (2, (4, 4, 16)), (2, (5, 7, 18)), (1, (4, 4, 16))], ids=["5x7x18_N1", "4x4x16_N2", "5x7x18_N2", "4x4x16_N1"])
@pytest.mark.parametrize("circular", [False, True], ids=["zeros", "circ"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("cout", [16, 32])
@pytest.mark.parametrize("cin", [3, 4])
def test_conv_in_forward_and_weight_gradient_exact_integers(cin, cout, dtype, circular, n, grid):
    """conv_in through hip_ops.Conv on exact integers against float64 F.conv3d and its autograd, bit for bit.
    Forward: x in {-2..2}, W in {-1, 0, 1}, bias in {-2..2}: |any partial sum| <= 2 * 27 * cin + 2 <= 218 < 2^8, so the bf16 re-rounding
    of the output (bf16 storage) is exact too.  Weight gradient: x, dout in {-2..2} over at most 2 * 5 * 7 * 18 = 1260 voxels: sums below
    4 * 1260 < 2^24 (fp32 outputs, no re-rounding); the bias gradient is the sum of dout."""
    _lib, ops = _mods()
    d, h, w = grid
    assert 2 * 27 * cin + 2 < 2 ** 8 and 4 * n * d * h * w < 2 ** 24
    x = _small_ints((n, d, h, w, cin), 71, -2, 2)
    wt = _small_ints((27, cout, cin), 72, -1, 1)
    bias = _small_ints((cout,), 73, -2, 2)
    dout = _small_ints((n, d, h, w, cout), 74, -2, 2)
    # reference: float64 conv3d + autograd
    x64 = x.double().permute(0, 4, 1, 2, 3)
    w64 = wt.double().view(3, 3, 3, cout, cin).permute(3, 4, 0, 1, 2).contiguous().requires_grad_(True)
    b64 = bias.double().requires_grad_(True)
    y64 = F.conv3d(F.pad(x64, (1,) * 6, mode="circular"), w64, b64) if circular else F.conv3d(x64, w64, b64, padding=1)
    y64.backward(dout.double().permute(0, 4, 1, 2, 3))
    ref_y = y64.detach().permute(0, 2, 3, 4, 1)
    ref_dw = w64.grad.permute(2, 3, 4, 0, 1).reshape(27, cout, cin)
    assert ref_y.abs().max().item() < 2 ** 8 and ref_dw.abs().max().item() < 2 ** 24
    # the plan of the weight gradient is the generic kernel (no thin-input kernel at cin > 2), so the fused GroupNorm tail is off
    conv = ops.Conv(cin, cout, 3, circular=circular)
    info = _lib.WgradPlanInfo()
    import ctypes
    _lib.check(_lib.lib().vdm_conv_wgrad_plan(conv.desc(n, d, h, w, dtype), 1, 0, ctypes.byref(info)), "vdm_conv_wgrad_plan")
    assert info.kernel != _lib.WGRAD_THIN_IN
    xd = _padded_dev(x, dtype, ops.cpad(cin, dtype))
    dd = _padded_dev(dout, dtype, ops.cpad(cout, dtype))
    assert not ops.gn_tail_ok(conv, dd)
    conv.pack(wt.to(DEV), dtype, need_dgrad=False)
    y = conv.fwd(xd, bias.to(DEV))
    assert y.dtype == dtype and y.shape == (n, d, h, w, ops.cpad(cout, dtype))
    assert_same_bits(y[..., :cout].float(), ref_y, "conv_in forward")
    dw = torch.full((27, cout, cin), float("nan"), device=DEV)
    db = torch.full((cout,), float("nan"), device=DEV)
    conv.wgrad(xd, dd, dw, db)
    assert_same_bits(dw, ref_dw, "conv_in weight gradient [tap, cout, cin]")
    assert_same_bits(db, b64.grad, "conv_in bias gradient")
