"""Kernel-level parity tests of the three input-gradient kernels, each alone through its hip_ops wrapper:
  K1t vdm_conv_in_dgrad (ops.conv_in_dgrad), K7b vdm_schedule_grad_sums (ops.schedule_grad_sums), K6i vdm_cond_input_grad
  (ops.CondTable.backward(dinputs=...)).

Two kinds of check, because they catch different faults:
  A. exact integers: operands are small integers held as floats, so every product and every partial sum is an integer below 2^24 and
     fp32 addition is exact in any order (and the values are exact in bf16 storage).  The kernel must `torch.equal` the same sum
     computed in float64 / int64 on the CPU: indexing, halo, wrap, tail and dropped or duplicated elements show with no tolerance.
  B. random reals against the same operation in torch float64, from inputs rounded to the storage type first, with a bound derived
     from the fp32 arithmetic (stated per kernel below) - never fitted to what the kernel gives.

K6i cannot be held to a closed-form bound (fp32 argument 1000 t f_i of sin / cos, device sinf / erff): its bound is measured against
the reference, not the kernel: e32 = max|oracle fp32 - oracle float64| per gradient tensor (both on the CPU), and the kernel must stay
within K6I_FACTOR * e32 + 2^-20 * max|oracle float64| (K6I_FACTOR_T for dL/dt: the reason stands next to it).

K6i, measured max over the gradient tensors of err / (factor * e32 + floor) on an MI355X (rows B = 1 / 4 / 7):
  chs0=16 t_only      0.172 / 0.218 / 0.266
  chs0=16 v_only_6_3  0.069 / 0.105 / 0.087
  chs0=16 t_and_6     0.219 / 0.246 / 0.209
  chs0=16 t_and_5_1   0.231 / 0.157 / 0.161
  chs0=48 t_only      0.170 / 0.183 / 0.183
  chs0=48 v_only_6_3  0.165 / 0.096 / 0.097
  chs0=48 t_and_6     0.152 / 0.161 / 0.132
  chs0=48 t_and_5_1   0.167 / 0.171 / 0.150
  chs0=64 t_only      0.213 / 0.422 / 0.227
  chs0=64 v_only_6_3  0.081 / 0.078 / 0.113
  chs0=64 t_and_6     0.166 / 0.194 / 0.199
  chs0=64 t_and_5_1   0.208 / 0.182 / 0.155
  (worst dL/dt tensor 0.422 with K6I_FACTOR_T = 32 - it was 1.425 with 8, see K6I_FACTOR_T; worst other tensor 0.266 with K6I_FACTOR = 8)
"""
import math

import pytest
import torch
import torch.nn.functional as F

from _exact import assert_same_bits, in_sentinel, ints

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U32 = 2.0 ** -24                      # unit roundoff of fp32


def _ops():
    from vdm4cdm_amd import hip_ops
    return hip_ops


def rnd(shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * scale
    return x.to(dtype).float()          # value representable in `dtype`, held as fp32 on the CPU


# =============================================================================================== K1t: conv_in's input gradient
def ref_conv_in_dgrad(dh, weight, cin, circular, dtype=torch.float64):
    """dh [N, D, H, W, C], weight [27, C, cin] (the layout of ref_conv in test_kernels_gpu.py) -> the gradient of conv_in's input,
    [N, cin, D, H, W]: autograd of F.conv3d at a zero input."""
    n, d, h, w, c = dh.shape
    x = torch.zeros(n, cin, d, h, w, dtype=dtype, requires_grad=True)
    wt = weight.to(dtype).view(3, 3, 3, c, cin).permute(3, 4, 0, 1, 2)
    y = F.conv3d(F.pad(x, (1,) * 6, mode="circular"), wt) if circular else F.conv3d(x, wt, padding=1)
    y.backward(dh.to(dtype).permute(0, 4, 1, 2, 3))
    return x.grad


K1T_RAGGED = [(5, 7, 18), (6, 9, 20)]                             # ragged in every axis (output tile 4 x 4 x 16)
K1T_TINY = [(1, 1, 1), (2, 2, 2), (1, 5, 3)]                      # every dimension below the halo: circular padding wraps onto itself
K1T_OTHER = [(4, 4, 16), (8, 8, 32), (3, 4, 33), (17, 3, 16)]     # one exact tile, exact multiple, one voxel into a third x tile, H < tile
K1T_BELOW_TILE = K1T_TINY + [(3, 4, 33), (17, 3, 16)]


def _k1t_cases():
    """Every (C, cin, storage, padding) combination gets three grids: one ragged, one tiny, one of the others; the grids and the batch
    size rotate with co-prime strides so that every grid meets both paddings, both storage types and both cin."""
    cases, i = [], 0
    for C in (16, 32, 48, 64):
        for cin in (1, 2):
            for dtype in (torch.float32, torch.bfloat16):
                for circular in (False, True):
                    r = i // 2 + (i % 2) * 5          # the two paddings of one (C, cin, storage) take different grids
                    grids = [(K1T_RAGGED[r % 2], 3 if (r // 2) % 2 == 0 else 1), (K1T_TINY[r % 3], 1 if r % 2 == 0 else 3),
                             (K1T_OTHER[(r + i // 8) % 4], 1 if (r // 4) % 2 == 0 else 3)]
                    for grid, n in grids:
                        cases.append((C, cin, dtype, circular, grid, n))
                    i += 1
    return cases


def _k1t_id(c):
    C, cin, dtype, circular, (d, h, w), n = c
    return f"C{C}_cin{cin}_{'f32' if dtype == torch.float32 else 'bf16'}_{'circ' if circular else 'zeros'}_{d}x{h}x{w}_N{n}"


K1T_CASES = _k1t_cases()


def test_k1t_case_table_covers_the_issue():
    combos = {}
    for C, cin, dtype, circular, grid, n in K1T_CASES:
        combos.setdefault((C, cin, dtype, circular), []).append((grid, n))
    assert len(combos) == 32
    for key, gs in combos.items():
        assert any(g in K1T_RAGGED for g, _ in gs) and any(g in K1T_BELOW_TILE for g, _ in gs), key
    for grid in K1T_RAGGED + K1T_TINY + K1T_OTHER:
        seen = [(dtype, circular, cin, n) for _, cin, dtype, circular, g, n in K1T_CASES if g == grid]
        assert {s[0] for s in seen} == {torch.float32, torch.bfloat16} and {s[1] for s in seen} == {False, True}, grid
        assert {s[2] for s in seen} == {1, 2} and {s[3] for s in seen} == {1, 3}, grid
    assert any(g in K1T_RAGGED and n == 3 for *_, g, n in K1T_CASES)          # the n decode of blockIdx.x on a ragged grid


def _k1t_run(dh, weight, cin, dtype, circular):
    ops = _ops()
    dz, ds = ops.conv_in_dgrad(dh.to(dtype).to(DEV).contiguous(), weight.to(DEV), cin, circular, want_s=(cin == 2))
    assert dz.dtype == torch.float32 and (ds is None) == (cin == 1)
    return torch.stack([dz] if cin == 1 else [dz, ds], dim=1).cpu()          # [N, cin, D, H, W] like the reference


@pytest.mark.parametrize("case", K1T_CASES, ids=_k1t_id)
def test_k1t_exact_integers(case):
    """Check A: dh and W uniform in {-2..2}: every partial sum is an integer of magnitude <= 4 * 27 * C = 6912 at most, so the kernel
    must give the bits of the float64 transposed convolution."""
    C, cin, dtype, circular, (d, h, w), n = case
    dh, wt = ints((n, d, h, w, C), 11, terms=27 * C), ints((27, C, cin), 12, terms=27 * C)
    assert_same_bits(_k1t_run(dh, wt, cin, dtype, circular), ref_conv_in_dgrad(dh, wt, cin, circular), _k1t_id(case))


@pytest.mark.parametrize("case", K1T_CASES, ids=_k1t_id)
def test_k1t_random_against_float64(case):
    """Check B, per output voxel q: |got - ref64| <= (27 C + 1) 2^-24 S(q), S = the same transposed convolution of |dh| and |W|: the
    running-error bound of an fp32 dot product of 27 C terms in any order.  bf16 storage adds nothing (bf16 -> fp32 is exact, the
    weights are the fp32 masters, the outputs fp32).  Loose (torch's own fp32 conv sits near 0.006 of it) but local: it scales with
    the magnitude around each voxel; check A carries the sharp edge."""
    C, cin, dtype, circular, (d, h, w), n = case
    dh, wt = rnd((n, d, h, w, C), 21, dtype), rnd((27, C, cin), 22, scale=0.2)
    got = _k1t_run(dh, wt, cin, dtype, circular).double()
    ref = ref_conv_in_dgrad(dh, wt, cin, circular)
    bound = (27 * C + 1) * U32 * ref_conv_in_dgrad(dh.abs(), wt.abs(), cin, circular)
    err = (got - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"K1t B {_k1t_id(case)}: max err {err.max().item():.3e}, worst err/bound {worst:.4f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), f"worst err / bound {worst} at {(err / bound.clamp_min(1e-300)).argmax().item()}"


@pytest.mark.parametrize("name,C,n,grid,circular", [("bench_128", 32, 2, (128, 128, 128), False), ("ragged_50x60x70", 48, 1, (50, 60, 70), True)],
                         ids=["bench_128_zeros", "ragged_50x60x70_circ"])
def test_k1t_exact_integers_large(name, C, n, grid, circular):
    """Check A at the bench shape and at a large ragged circular grid (bf16 storage, cin = 2)."""
    d, h, w = grid
    dh, wt = ints((n, d, h, w, C), 31, terms=27 * C), ints((27, C, 2), 32, terms=27 * C)
    # the reference runs torch's fp32 conv: on these inputs it is exact too (integer partial sums below 2^24 in any order), and the
    # float64 conv of a 128^3 batch would only cost time
    ref = ref_conv_in_dgrad(dh, wt, 2, circular, dtype=torch.float32)
    assert_same_bits(_k1t_run(dh, wt, 2, torch.bfloat16, circular), ref, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("circular", [False, True], ids=["zeros", "circ"])
def test_k1t_without_ds_and_repeatable(dtype, circular):
    """want_s=False with cin = 2 (ds NULL): dz has the bits of the want_s=True call; a second launch repeats both outputs bit for bit."""
    ops = _ops()
    for k, (n, grid, C) in enumerate([(3, (5, 7, 18), 48), (1, (1, 5, 3), 16), (2, (3, 4, 33), 64)]):
        dh = rnd((n,) + grid + (C,), 40 + k, dtype).to(dtype).to(DEV)
        wt = rnd((27, C, 2), 50 + k, scale=0.2).to(DEV)
        dz, ds = ops.conv_in_dgrad(dh, wt, 2, circular, want_s=True)
        dz0, none = ops.conv_in_dgrad(dh, wt, 2, circular, want_s=False)
        assert none is None and torch.equal(dz0, dz)
        dz2, ds2 = ops.conv_in_dgrad(dh, wt, 2, circular, want_s=True)
        assert torch.equal(dz2, dz) and torch.equal(ds2, ds)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("circular", [False, True], ids=["zeros", "circ"])
@pytest.mark.parametrize("n,grid", [(3, (5, 7, 18)), (1, (1, 1, 1)), (2, (3, 4, 33))], ids=["ragged", "one_voxel", "third_x_tile"])
def test_k1t_cin1_writes_dz_only(dtype, circular, n, grid):
    """cin = 1: dz is the only output; it is a slice of a sentinel-filled buffer here (the C entry directly: the wrapper allocates dz
    itself), and the sentinels on both sides survive while the slice holds the exact integers."""
    from vdm4cdm_amd import _lib
    ops = _ops()
    C = 32
    d, h, w = grid
    dh, wt = ints((n, d, h, w, C), 61, terms=27 * C), ints((27, C, 1), 62, terms=27 * C)
    dh_d, wt_d = dh.to(dtype).to(DEV).contiguous(), wt.to(DEV)
    buf, dz, untouched = in_sentinel(n * d * h * w, (n, d, h, w))
    _lib.check(_lib.lib().vdm_conv_in_dgrad(dh_d.data_ptr(), n, d, h, w, C, ops.dt_id(dtype), _lib.PAD_CIRCULAR if circular else _lib.PAD_ZEROS,
                                            wt_d.data_ptr(), 1, dz.data_ptr(), None, None), "vdm_conv_in_dgrad")
    torch.cuda.synchronize()
    assert untouched(), "conv_in_dgrad wrote outside dz"
    assert_same_bits(dz.cpu()[:, None], ref_conv_in_dgrad(dh, wt, 1, circular), "dz inside the sentinel buffer")


# =============================================================================================== K7b: the schedule's per-sample sums
K7B_PERS = [4, 4 * 255, 4 * 256, 4 * 257, 840, 20 ** 3, 4 * 4096 * 3 + 4]      # one group; the block boundary of the first stride;
K7B_CASES = [(n, per) for n in (1, 2, 3, 7) for per in K7B_PERS] + [(2, 128 ** 3)]   # n4 = 210; 20^3; several blocks + a one-group tail; bench


def _k7b_ref(dz, x, eps):
    dz, x, eps = dz.double(), x.double(), eps.double()
    return torch.stack([(dz * x).sum(1), (dz * eps).sum(1)], dim=1)


@pytest.mark.parametrize("n,per", K7B_CASES, ids=[f"n{n}_per{p}" for n, p in K7B_CASES])
def test_k7b_exact_integers(n, per):
    """Check A: dz, x, eps uniform in {-2..2}: partial sums are integers below 4 * per <= 2^23, so both columns equal the int64 sums."""
    ops = _ops()
    dz, x, eps = (ints((n, per), 70 + k, terms=per) for k in range(3))
    ref = torch.stack([(dz.long() * x.long()).sum(1), (dz.long() * eps.long()).sum(1)], dim=1)
    got = ops.schedule_grad_sums(dz.to(DEV), x.to(DEV), eps=eps.to(DEV))
    assert got.shape == (n, 2) and got.dtype == torch.float32
    assert_same_bits(got, ref, f"sums n={n} per={per}")


@pytest.mark.parametrize("n,per", K7B_CASES, ids=[f"n{n}_per{p}" for n, p in K7B_CASES])
def test_k7b_random_against_float64(n, per):
    """Check B: the sum is a tree (thread-serial, wave, block, fold) whose depth is not part of the interface, so the bound is the
    order-independent one: |err_n| <= per 2^-24 sum_i |dz_i x_i| (the same with eps).  It is loose at 128^3 (per 2^-24 = 1/8): check A
    is what pins every element's inclusion; this one catches a sum carried in the wrong type or a wrong operand."""
    ops = _ops()
    dz, x, eps = (rnd((n, per), 80 + k) for k in range(3))
    got = ops.schedule_grad_sums(dz.to(DEV), x.to(DEV), eps=eps.to(DEV)).cpu().double()
    ref = _k7b_ref(dz, x, eps)
    bound = per * U32 * _k7b_ref(dz.abs(), x.abs(), eps.abs())
    err = (got - ref).abs()
    print(f"K7b B n={n} per={per}: max err {err.max().item():.3e}, worst err/bound {(err / bound).max().item():.5f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), (err, bound)


@pytest.mark.parametrize("seed,stream_id", [(1234, 3), ((1 << 40) + 12345, 7)], ids=["seed_small", "seed_above_2_32"])
@pytest.mark.parametrize("per", [4 * 257, 840, 4 * 4096 * 3 + 4])
def test_k7b_regenerated_noise_is_the_randn_field(seed, stream_id, per):
    """eps = None regenerates the field ops.randn(seed, stream_id) writes - same kernel, same order, so the same bits as supplying that
    field; another stream id gives another field.  Column 1 is asserted sample by sample, against the supplied call and against the
    float64 sum over that sample's slice of the whole [3, per] field, so a wrong n * n4 + i Philox offset names the sample."""
    ops = _ops()
    n = 3
    dz, x = rnd((n, per), 90).to(DEV), rnd((n, per), 91).to(DEV)
    field = ops.randn(torch.empty_like(x), seed, stream_id)
    regen = ops.schedule_grad_sums(dz, x, eps=None, seed=seed, stream_id=stream_id)
    supplied = ops.schedule_grad_sums(dz, x, eps=field)
    ref = _k7b_ref(dz.cpu(), x.cpu(), field.cpu())
    bound = per * U32 * _k7b_ref(dz.cpu().abs(), x.cpu().abs(), field.cpu().abs())
    for s in range(n):
        assert regen[s, 1].item() == supplied[s, 1].item(), f"sample {s}: regenerated {regen[s, 1].item()} != supplied {supplied[s, 1].item()}"
        assert abs(regen[s, 1].item() - ref[s, 1].item()) <= bound[s, 1].item(), f"sample {s}: not the sum over its slice of the field"
        one = ops.schedule_grad_sums(dz[s:s + 1], x[s:s + 1], eps=field[s:s + 1])         # the slice on its own (n = 1: same blocks per sample)
        assert one[0, 1].item() == regen[s, 1].item(), f"sample {s}: sliced field {one[0, 1].item()} != regenerated {regen[s, 1].item()}"
    assert torch.equal(regen, supplied)
    other = ops.schedule_grad_sums(dz, x, eps=None, seed=seed, stream_id=stream_id + 1)
    assert torch.equal(other[:, 0], regen[:, 0]) and (other[:, 1] != regen[:, 1]).all()
    low = ops.schedule_grad_sums(dz, x, eps=None, seed=seed & 0xffffffff, stream_id=stream_id)
    if seed >> 32:
        assert (low[:, 1] != regen[:, 1]).all(), "the high half of the seed is ignored"


def test_k7b_seed_step_counter():
    """ops.SEED_STEP (the device counter a captured training step mixes into every seed): regenerated and supplied sums still agree
    when ops.randn ran under the same counter, and differ from the counter = 0 result."""
    ops = _ops()
    n, per, seed, sid = 3, 840, 99, 2
    dz, x = rnd((n, per), 95).to(DEV), rnd((n, per), 96).to(DEV)
    assert ops.SEED_STEP is None
    try:
        results = {}
        for step in (0, 5):
            ops.SEED_STEP = torch.tensor([step], dtype=torch.int32, device=DEV)
            field = ops.randn(torch.empty_like(x), seed, sid)
            regen = ops.schedule_grad_sums(dz, x, eps=None, seed=seed, stream_id=sid)
            assert torch.equal(regen, ops.schedule_grad_sums(dz, x, eps=field)), f"counter {step}"
            ref = _k7b_ref(dz.cpu(), x.cpu(), field.cpu())
            assert ((regen.cpu().double() - ref).abs() <= per * U32 * _k7b_ref(dz.cpu().abs(), x.cpu().abs(), field.cpu().abs())).all()
            results[step] = (regen, field)
    finally:
        ops.SEED_STEP = None
    assert torch.equal(results[0][0][:, 0], results[5][0][:, 0]) and (results[0][0][:, 1] != results[5][0][:, 1]).all()
    assert not torch.equal(results[0][1], results[5][1])
    assert torch.equal(results[0][1], ops.randn(torch.empty_like(x), seed, sid))          # counter 0 = no counter


def test_k7b_repeatable_at_bench_shape():
    ops = _ops()
    n, per = 2, 128 ** 3
    dz, x, eps = (rnd((n, per), 100 + k).to(DEV) for k in range(3))
    a, b = ops.schedule_grad_sums(dz, x, eps=eps), ops.schedule_grad_sums(dz, x, eps=eps)
    assert torch.equal(a, b)
    a, b = ops.schedule_grad_sums(dz, x, seed=5, stream_id=1), ops.schedule_grad_sums(dz, x, seed=5, stream_id=1)
    assert torch.equal(a, b)


# =============================================================================================== K6i: conditioning input gradients
K6I_FACTOR = 8          # device summation order and device sinf / cosf / erff against the CPU's, see the module docstring
# dL/dt alone gets a larger factor.  With 8 its worst measured ratio was 1.425 (chs0 = 64, t only, B = 4, the row t = 1: err 2.95e-3 on
# |dL/dt| = 452, e32 = 2.05e-4) while no other tensor of any configuration passed 0.27.  Cause, from the per-frequency breakdown of that
# row: dL/dt is a signed sum of 64 terms g_i 1000 f_i [cos, -sin](1000 t f_i) in which a handful of low frequencies (i = 1..5) each
# carry about 1e-3 of error from the rounding of the fp32 argument alone; on the device every one of them is within one ulp of the
# argument (0.3 .. 0.93 x arg 2^-24), as on the CPU, but the CPU's happen to cancel (+8.4e-4 - 8.0e-4 - 6.8e-4 + 2.8e-4) while the
# device's expf rounds f_3 the other way (+1.8e-3).  e32 of a tensor of B values is one draw of that cancellation (it moves by 10x
# between two host CPUs for the same configuration), not the scale of an honest fp32 error, which is the sum of the magnitudes
# (3 - 4e-3 here).  The kernel is right; 4 x 8 covers the cancellation; worst measured ratio of dL/dt with 32: 0.422.
K6I_FACTOR_T = 32
K6I_CONDS = {"t_only": (True, ()), "v_only_6_3": (False, (6, 3)), "t_and_6": (True, (6,)), "t_and_5_1": (True, (5, 1))}
K6I_T_VALUES = [1.0, 0.0, 1e-4, 0.5]          # the endpoints are where sin / cos saturate; the argument reaches 1000 at t = 1


def sinusoidal_embedding_f64(t, dim=64):
    """oracle.unet_oracle.sinusoidal_embedding restated in float64 (the oracle's casts to fp32 inside)."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    args = 1000.0 * t[:, None] * freqs[None, :]
    return torch.cat([torch.sin(args), torch.cos(args)], dim=1)


def _k6i_setup(chs0, cond, B, seed=5):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from helpers import oracle_params, randomize
    from vdm4cdm_amd.networks import CUNet
    has_t, vd = K6I_CONDS[cond]
    net = CUNet(shape=(1, 16, 16, 16), chs=[chs0, 2 * chs0], s_conditioning_channels=0, v_conditioning_dims=list(vd), t_conditioning=has_t,
                norm_groups=8, backend="hip", precision="fp32")
    randomize(net, seed)
    g = torch.Generator().manual_seed(1)
    t = torch.cat([torch.tensor(K6I_T_VALUES[:B]), torch.rand(max(B - len(K6I_T_VALUES), 0), generator=g)])
    vs = [torch.randn(B, d, generator=g) for d in vd]
    dtab = torch.randn(B, net.table_width, generator=g)
    P = {k: v for k, v in oracle_params(net).items() if "embed" in k or ".cond." in k}
    return net, (t if has_t else None), vs, dtab, P


def _k6i_oracle(net, P, t, vs, dtab, dtype):
    """The oracle's sinusoidal_embedding / _mlp2 / per-block F.linear in `dtype` from the fp32 parameters and inputs; returns the
    gradients of the inputs (t first) and of the parameters."""
    from oracle import unet_oracle
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    leaves, conds = [], []
    if t is not None:
        tl = t.to(dtype).clone().requires_grad_(True)
        leaves.append(tl)
        emb = sinusoidal_embedding_f64(tl) if dtype == torch.float64 else unet_oracle.sinusoidal_embedding(tl)
        assert emb.dtype == dtype
        conds.append(unet_oracle._mlp2(p, "t_embed", emb))
    for k, v in enumerate(vs):
        vl = v.to(dtype).clone().requires_grad_(True)
        leaves.append(vl)
        conds.append(unet_oracle._mlp2(p, f"v_embeds.{k}", vl))
    table = torch.cat([sum(F.linear(c, p[f"{b.name}.cond.{k}.weight"]) for k, c in enumerate(conds)) for b in net.blocks], dim=1)
    assert table.dtype == dtype
    table.backward(dtab.to(dtype))
    return [l.grad.double() for l in leaves], {k: v.grad.double() for k, v in p.items()}


def k6i_reference(net, P, t, vs, dtab):
    """(float64 gradients, e32 per tensor) with e32 = max|oracle fp32 - oracle float64|: what an honest fp32 implementation of the same
    formulas loses; the kernel's bound is factor * e32 + 2^-20 * max|float64 gradient| per tensor."""
    din64, dp64 = _k6i_oracle(net, P, t, vs, dtab, torch.float64)
    din32, dp32 = _k6i_oracle(net, P, t, vs, dtab, torch.float32)
    e_in = [(a - b).abs().max().item() for a, b in zip(din32, din64)]
    e_p = {k: (dp32[k] - dp64[k]).abs().max().item() for k in dp64}
    return din64, dp64, e_in, e_p


def _k6i_run(net, t, vs, dtab, want=None, scale=1.0):
    """forward + backward of the table on the device; want: which dinputs to ask for (None = no dinputs argument at all).  Returns
    (dinputs list with None where not asked, the flat gradient vector, sentinel checks)."""
    ops = _ops()
    B = dtab.shape[0]
    flat = net.flat.detach().to(DEV)
    specs = net.cond_specs(None if t is None else t.to(DEV), [v.to(DEV) for v in vs], flat)
    ct = ops.CondTable(specs, B, net.table_width)
    ct.forward(save=True)
    gflat = torch.full_like(flat, float("nan"))
    grads = [{k: sp[k] for k in ("w1", "b1", "w2", "b2", "wproj")} for sp in net.cond_specs(None, [None] * len(vs), gflat)]
    dpad = torch.zeros(B, net.table_width + 7, device=DEV)          # row stride != width
    dpad[:, :net.table_width] = (scale * dtab).to(DEV)
    dins, checks = None, []
    if want is not None:
        dins = []
        for sp, w in zip(specs, want):
            if not w:
                dins.append(None)
                continue
            _, view, untouched = in_sentinel(sp["input"].numel(), tuple(sp["input"].shape), pad=32)
            dins.append(view)
            checks.append(untouched)
    ct.backward(dpad[:, :net.table_width], grads, dinputs=dins)
    torch.cuda.synchronize()
    return dins, gflat, checks


K6I_CASES = [(chs0, cond, B) for chs0 in (16, 48, 64) for cond in K6I_CONDS for B in (1, 4, 7)]


@pytest.mark.parametrize("chs0,cond,B", K6I_CASES, ids=[f"chs{c}_{k}_B{b}" for c, k, b in K6I_CASES])
def test_k6i_input_gradients(chs0, cond, B):
    """dL/dt and dL/dv of every conditioning, and the parameter gradients of the same call, against the float64 oracle within
    K6I_FACTOR * e32 + 2^-20 max|ref| per tensor (K6I_FACTOR_T for dL/dt); asking for input gradients leaves the parameter gradients
    bit-equal; the outputs sit in sentinel-filled buffers ([rows] for t, [rows, d] for a vector) whose sentinels survive."""
    from helpers import oracle_params
    net, t, vs, dtab, P = _k6i_setup(chs0, cond, B)
    din64, dp64, e_in, e_p = k6i_reference(net, P, t, vs, dtab)
    nspec = len(din64)
    _, gflat0, _ = _k6i_run(net, t, vs, dtab, want=None)
    dins, gflat, checks = _k6i_run(net, t, vs, dtab, want=[True] * nspec)
    assert all(c() for c in checks), "cond_input_grad wrote outside a dinputs tensor"
    assert torch.equal(torch.nan_to_num(gflat, nan=12345.0), torch.nan_to_num(gflat0, nan=12345.0)), \
        "asking for input gradients changed the parameter gradients"
    worst, lines = 0.0, []
    names = ["t"] * (t is not None) + [f"v{k}" for k in range(len(vs))]
    got_p = oracle_params(net, flat=gflat)
    items = [(names[k], dins[k].cpu().double(), din64[k], e_in[k]) for k in range(nspec)]
    items += [(n, got_p[n].double(), dp64[n], e_p[n]) for n in dp64]
    for name, got, ref, e32 in items:
        assert got.shape == ref.shape and torch.isfinite(got).all(), name
        err = (got - ref).abs().max().item()
        tol = (K6I_FACTOR_T if name == "t" else K6I_FACTOR) * e32 + 2.0 ** -20 * ref.abs().max().item()
        ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        lines.append(f"  {name}: err {err:.3e} e32 {e32:.3e} max|ref| {ref.abs().max().item():.3e} ratio {ratio:.3f}")
    print(f"K6i chs0={chs0} {cond} B={B}: worst ratio {worst:.3f}\n" + "\n".join(lines))
    assert worst <= 1.0, f"worst err / (factor e32 + floor) = {worst}\n" + "\n".join(lines)


K6I_MULTI = [(chs0, cond, B) for chs0 in (16, 48, 64) for cond in ("v_only_6_3", "t_and_6", "t_and_5_1") for B in (4, 7)]


@pytest.mark.parametrize("chs0,cond,B", K6I_MULTI, ids=[f"chs{c}_{k}_B{b}" for c, k, b in K6I_MULTI])
def test_k6i_none_entries_and_linearity(chs0, cond, B):
    """A None entry of dinputs (gradient wanted for one conditioning and not another, each way round) leaves the others bit-equal and
    writes nothing beside them.  And with no tolerance at all: d input is linear in dtable, so dtable * 2 doubles every input gradient
    exactly (a power-of-two scaling is exact in fp32) and -dtable negates it."""
    net, t, vs, dtab, P = _k6i_setup(chs0, cond, B)
    nspec = (t is not None) + len(vs)
    full, _, checks = _k6i_run(net, t, vs, dtab, want=[True] * nspec)
    assert all(c() for c in checks)
    for k in range(nspec):
        for want in ([j == k for j in range(nspec)], [j != k for j in range(nspec)]):
            part, _, checks = _k6i_run(net, t, vs, dtab, want=want)
            assert all(c() for c in checks), f"want={want}: wrote outside a dinputs tensor"
            for j in range(nspec):
                assert (part[j] is None) == (not want[j])
                if want[j]:
                    assert torch.equal(part[j], full[j]), f"want={want}: dinputs[{j}] changed"
    twice, _, _ = _k6i_run(net, t, vs, dtab, want=[True] * nspec, scale=2.0)
    minus, _, _ = _k6i_run(net, t, vs, dtab, want=[True] * nspec, scale=-1.0)
    for j in range(nspec):
        assert full[j].abs().max().item() > 0
        assert_same_bits(twice[j], 2.0 * full[j], f"dinputs[{j}] for 2 * dtable")
        assert_same_bits(minus[j], -full[j], f"dinputs[{j}] for -dtable")
