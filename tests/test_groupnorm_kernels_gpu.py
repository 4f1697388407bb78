"""Kernel-level parity tests of the GroupNorm family: vdm_gn_stats (full pass and from conv tile partials), gn_silu_fwd, gn_dyh,
gn_bwd_finalize, gn_bwd_apply, channel_sums / channel_dot_sums, the skip-fused passes (csrc/gn_skip.hip), the folded
backward of the conv kernels, and the wgrad_thin tail.  Two kinds of check, as in tests/test_input_grad_kernels_gpu.py:

A. exact integers.  Operands are integers in {-2..2} held in the storage type; every sum stays below 2^24, so fp32 addition is exact in
   any order and the kernel must `torch.equal` the int64 / float64 sum on the CPU: indexing, group offsets (g0), the concat boundary,
   ragged sweeps, dropped or duplicated elements show with no tolerance.  A1 full statistics pass, A2 statistics from conv partials
   (selector convs: one +-1 weight per output channel, so the conv output is an exact shifted copy), A3 channel sums, A4 dbeta through
   the finalize + apply kernels, A5 the dropout bits of forward, mask bytes and backward.

B. random reals against float64 (tests/_gn_bounds.py; reference = F.group_norm / F.silu and autograd in float64 - test_groupnorm_cpu.py
   shows that the formulas there are exactly those - from inputs rounded to the storage type first), with a bound DERIVED from the fp32
   arithmetic of the raw-moment formulation, never fitted to the kernels.

Derivation.  u = 2^-24; per (sample, group): m, q, v = float64 mean, mean square, variance, rho = (v + eps)^-1/2, a1 = mean |x|; d = the
longest chain of fp32 additions one element passes through on its way into {sum, sumsq} (thread sweep + butterfly + LDS fold + the two
finalize folds: _gn_bounds.stats_chain counts it from the code per case; d <= 64 in every case but one, B_CASES lists them).
  sums       |d sum| <= d u sum|x|,  |d sumsq| <= (d + 1) u sumsq          (running-error bound of a sum in any fixed order)
  mean       |dm|  <= (d + 1) u a1                                          (the division adds u)
  variance   |dv|  <= (d + 2) u q + 2 |m| |dm| + 2 u m^2 + u v  =: Ev       (q^ = sumsq / cnt, the square of m^, its rounding, the
                                                                             subtraction; max(., 0) only moves v^ towards v >= 0)
  rstd       |drho| <= 1/2 rho*^3 Ev + 4 u rho*,  rho* = (max(v - Ev, 0) + eps)^-1/2      (mean-value theorem with the steepest slope
                                                                             in reach; the addition of eps and v_rsq_f32's ulp)
  y_lin      |dy_lin| <= |gamma| (|x - m| |drho| + rho* |dm|) + 4 u (|x gamma rho*| + |m gamma rho*| + |beta|)
                                                                            (A = rho gamma, B = beta - m A, x A + B: one u each)
  y = silu   |dy| <= 1.1 |dy_lin| + u |silu(y_lin)| (8 + 2 (1 - sigma) |y_lin|)          (sup |silu'| = 1.0998; the device evaluates
             y rcp(1 + __expf(-y)): exp2 of a rounded product, relative error 2u (|y| + 2), damped by 1 - sigma on its way into
             sigma; the addition, the reciprocal (2u) and the product)
  storage    bf16 output: + 2^-8 |y^| (round to nearest, 8 significant bits); fp32: nothing.
The Ev term carries the conditioning: Ev ~ (d + 6) u m^2 for |m| >> std, so |drho| / rho ~ (d + 6) u (m / std)^2 / 2.

Backward.  dyh = dy silu'(y_lin) (gn_dyh; `linear`: dyh = dy):  |d dyh| <= |dy| (1/2 |dy_lin| + E') + u |dyh| (+ storage), sup |silu''| =
1/2, E' the evaluation error of s (1 + y (1 - s)) (_gn_bounds.dsilu_eval_err).  Behind dyh, with T1_c = sum_v dyh, T2_c = sum_v dyh x
(chains of d1 additions, e1 = d1 u sum|dyh| + sum|d dyh|, e2 = (d1 + 1) u sum|dyh x| + sum|d dyh| |x|), Tx_c = rho (T2 - m T1):
  |dTx|  <= |drho| |T2 - m T1| + rho* (e2 + |m| e1 + |dm| |T1| + u |m T1| + u |T2 - m T1|) + u |Tx|     (u |m T1|: the cancellation
                                                                             of T2 - m T1 at a large mean)
  dbeta  = sum_n T1:  sum_n e1 + (n - 1) u sum_n |T1|;   dgamma = sum_n Tx likewise with dTx
  m1, m2 = sum_c gamma (T1, Tx) / cnt:  |dm_k| <= (sum_c |gamma| e_k + (gs + 1) u sum_c |gamma T_k|) / cnt + u |m_k|
  dx = P dyh + Q x + R,  P = rho gamma, Q = -rho^2 m2, R = rho (m rho m2 - m1)  =  rho (gamma dyh - m1 - xhat m2).  First order in the
  four parameter errors (the errors of m2 in Q and R cancel exactly as in the kernel: together they are -rho xhat dm2):
  |d dx| <= |drho| |gamma dyh - m1 - 2 xhat m2| + rho*^2 |m2| |dm| + rho* |dm1| + rho* |xhat| |dm2| + rho* |gamma| |d dyh|
            + u (2 |P dyh| + 2 |Q x| + 3 rho*^2 |m m2| + rho* |m rho m2 - m1| + |R| + |x Q + R| + |dx|)
  where 2 u |Q x| + 3 u rho*^2 |m m2| is the part that does NOT cancel: Q x and R are rounded on their own, each of size rho^2 |m m2|
  at a large mean while their sum is rho |xhat m2| - the u |m| rho^2 |m2| term.
  colsum = rho (gamma T1 - V m1 - m2 xhsum), xhsum = rho (chsum - V m): the same propagation with u V |m| for the cancellation in
  chsum - V m (_gn_bounds.bwd).  Residual gradients (add) and the skip conv's W^T dout are fp32 terms added before the store.
Conv-fused consumers: only the GroupNorm part is bounded.  The skip-fused forward and the wgrad_thin
tail must equal the unfused product path fed the same statistics bit for bit (as test_kernels_gpu.py establishes at offset 0.3);
Conv.dgrad_gn's dyh is compared with conv.dgrad's stored result times float64 silu'(y_lin), the two accumulation orders and the bf16
rounding of the plain result bounded by the conv's own running-error bound; its tile partials (fp32 values before the bf16 rounding,
chains of NV <= 8 rows + 4 + 3 inside a tile, then tile_partials_fold) feed gn_bwd_fused, bounded as above from the stored dyh.

Measured on an MI355X, max err / bound per consumer over B_CASES (rows |mean| / std = 0 / 1 / 4 / 16 / 64 / const_group / tiny_std /
mixed_offsets; bf16 outputs sit at the storage rounding of 2^-8, which the bound contains: near 1 by construction):
  fp32 storage
  fwd_silu          0.089 / 0.047 / 0.054 / 0.046 / 0.053 / 0.089 / 0.091 / 0.089
  fwd_linear        0.099 / 0.079 / 0.074 / 0.084 / 0.070 / 0.081 / 0.081 / 0.099
  bwd_silu_dx       0.073 / 0.042 / 0.034 / 0.026 / 0.030 / 0.073 / 0.073 / 0.058
  bwd_silu_dgamma   0.019 / 0.009 / 0.005 / 0.002 / 0.001 / 0.019 / 0.019 / 0.015
  bwd_silu_dbeta    0.023 / 0.014 / 0.015 / 0.015 / 0.022 / 0.023 / 0.023 / 0.023
  bwd_silu_colsum   0.010 / 0.008 / 0.007 / 0.010 / 0.003 / 0.010 / 0.010 / 0.011
  bwd_linear_dx     0.179 / 0.153 / 0.079 / 0.071 / 0.054 / 0.179 / 0.179 / 0.152
  bwd_linear_dgamma 0.047 / 0.024 / 0.031 / 0.029 / 0.045 / 0.047 / 0.047 / 0.047
  bwd_linear_dbeta  0.032 / 0.032 / 0.032 / 0.032 / 0.032 / 0.032 / 0.032 / 0.032
  bwd_linear_colsum 0.022 / 0.037 / 0.060 / 0.048 / 0.053 / 0.022 / 0.022 / 0.048
  dgrad_gn_dyh      0.022 / 0.016 / 0.024 / 0.025 / 0.041 / 0.017 / 0.017 / 0.031
  fold_dx           0.294 / 0.212 / 0.129 / 0.047 / 0.054 / 0.246 / 0.246 / 0.294
  fold_dgamma       0.016 / 0.010 / 0.014 / 0.027 / 0.041 / 0.015 / 0.015 / 0.028
  fold_dbeta        0.017 / 0.012 / 0.013 / 0.018 / 0.022 / 0.017 / 0.017 / 0.016
  fold_colsum       0.013 / 0.013 / 0.042 / 0.043 / 0.053 / 0.013 / 0.013 / 0.043
  bf16 storage
  fwd_silu          0.995 / 0.992 / 0.977 / 0.873 / 0.684 / 0.995 / 0.995 / 0.995
  fwd_linear        0.994 / 0.994 / 0.985 / 0.926 / 0.793 / 0.993 / 0.993 / 0.994
  bwd_silu_dx       0.832 / 0.842 / 0.774 / 0.704 / 0.499 / 0.832 / 0.832 / 0.832
  bwd_silu_dgamma   0.186 / 0.074 / 0.020 / 0.004 / 0.000 / 0.186 / 0.186 / 0.120
  bwd_silu_dbeta    0.167 / 0.136 / 0.151 / 0.079 / 0.039 / 0.167 / 0.167 / 0.094
  bwd_silu_colsum   0.077 / 0.082 / 0.070 / 0.042 / 0.009 / 0.077 / 0.077 / 0.059
  bwd_linear_dx     0.995 / 0.994 / 0.991 / 0.980 / 0.937 / 0.995 / 0.995 / 0.994
  bwd_linear_dgamma 0.035 / 0.018 / 0.017 / 0.022 / 0.032 / 0.035 / 0.035 / 0.032
  bwd_linear_dbeta  0.010 / 0.010 / 0.010 / 0.010 / 0.010 / 0.010 / 0.010 / 0.010
  bwd_linear_colsum 0.014 / 0.013 / 0.026 / 0.033 / 0.040 / 0.014 / 0.014 / 0.040
  skip_bwd_dx       0.993 / 0.993 / 0.988 / 0.972 / 0.951 / 0.993 / 0.993 / 0.991
  skip_bwd_dgamma   0.017 / 0.012 / 0.010 / 0.018 / 0.034 / 0.017 / 0.017 / 0.034
  skip_bwd_dbeta    0.002 / 0.002 / 0.002 / 0.002 / 0.002 / 0.002 / 0.002 / 0.002
  dgrad_gn_dyh      0.860 / 0.842 / 0.854 / 0.795 / 0.765 / 0.860 / 0.860 / 0.844
  fold_dx           0.895 / 0.886 / 0.870 / 0.808 / 0.777 / 0.895 / 0.895 / 0.895
  fold_dgamma       0.180 / 0.055 / 0.017 / 0.005 / 0.001 / 0.180 / 0.180 / 0.180
  fold_dbeta        0.105 / 0.127 / 0.118 / 0.120 / 0.097 / 0.105 / 0.105 / 0.090
  fold_colsum       0.070 / 0.080 / 0.079 / 0.051 / 0.032 / 0.070 / 0.070 / 0.080
(fwd = gn_silu_fwd; bwd = gn_silu_bwd: gn_dyh + channel_dot_sums + finalize + apply, with add1 / add2; skip_bwd = gn_bwd_fused(skip=...);
dgrad_gn_dyh / fold = Conv.dgrad_gn and the gn_bwd_fused behind it.  Absolute errors of the fp32 rows at |mean| / std = 0 / 1 / 4 / 16 / 64:
fwd_linear 7.4e-7 / 1.3e-6 / 1.8e-5 / 2.2e-4 / 3.7e-3, bwd_linear_dx 1.0e-6 / 1.5e-6 / 2.4e-5 / 3.6e-4 / 4.7e-3 - DESIGN.md, K2.)
"""
import math

import pytest
import torch

import _gn_bounds as B
from _exact import assert_same_bits, in_sentinel, ints
from test_kernels_gpu import GN_FUSED_CASES, ref_conv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]


def _ops():
    from vdm4cdm_amd import hip_ops
    return hip_ops


def _libmod():
    from vdm4cdm_amd import _lib
    return _lib


def tn(dtype):
    return "f32" if dtype == F32 else "bf16"


def dev(x, dtype):
    """CPU tensor of values representable in `dtype` -> contiguous device tensor of that type."""
    return x.float().to(dtype).to(DEV).contiguous()


def ref_stats(xs, G):
    """{sum, sumsq} per (sample, group) of the channel concat of xs in float64: [N, G, 2]."""
    x = torch.cat([t.double().reshape(t.shape[0], -1, t.shape[-1]) for t in xs], -1)
    xg = x.reshape(x.shape[0], x.shape[1], G, -1)
    return torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1)


def assert_exact_sums(st):
    assert st[..., 1].max().item() < 2 ** 24, "exact-integer check: a sum of squares reaches 2^24"


# =============================================================================================== A1: the full statistics pass
# dtype, n, voxel shape, c1, c2, groups.  PPV = channels of a source / (4 fp32 | 8 bf16).
A1_CASES = [
    # xor-butterfly path (64 % PPV == 0)
    (F32, 1, (3, 5, 7), 4, 0, 1), (F32, 3, (3, 5, 7), 8, 0, 8), (F32, 1, (1, 1, 1), 16, 0, 4), (F32, 3, (4, 6, 10), 32, 0, 32),
    (F32, 1, (3, 5, 7), 64, 0, 64), (F32, 3, (3, 5, 7), 128, 0, 2), (F32, 1, (4, 6, 10), 256, 0, 1),
    (BF16, 3, (3, 5, 7), 8, 0, 2), (BF16, 1, (3, 5, 7), 16, 0, 8), (BF16, 1, (1, 1, 1), 32, 0, 32), (BF16, 3, (4, 6, 10), 64, 0, 4),
    (BF16, 1, (3, 5, 7), 128, 0, 64), (BF16, 1, (3, 5, 7), 256, 0, 8), (BF16, 3, (3, 5, 7), 512, 0, 1),
    # generic path
    (BF16, 3, (3, 5, 7), 96, 0, 32), (BF16, 1, (3, 5, 7), 96, 0, 8), (BF16, 1, (4, 6, 10), 160, 0, 32), (BF16, 3, (3, 5, 7), 160, 0, 1),
    (F32, 3, (3, 5, 7), 96, 0, 32), (BF16, 1, (4, 6, 10), 192, 0, 64), (F32, 1, (3, 5, 7), 192, 0, 64), (BF16, 3, (3, 5, 7), 384, 0, 2),
    (F32, 3, (3, 5, 7), 512, 0, 1), (F32, 1, (1, 1, 1), 512, 0, 64), (F32, 1, (3, 5, 7), 48, 0, 4), (F32, 1, (3, 5, 7), 80, 0, 4),
    # every thread loops 8 times; the block count at its cap (864 wanted, 682 allowed)
    (F32, 2, (48, 48, 48), 32, 0, 8), (BF16, 2, (48, 48, 48), 32, 0, 8), (F32, 3, (48, 48, 48), 64, 0, 8),
    # two sources: unequal halves (64 + 32 needs a group size that divides 32: 6 or 12 groups), equal halves
    (F32, 1, (3, 5, 7), 64, 32, 12), (BF16, 3, (3, 5, 7), 64, 32, 6), (F32, 3, (3, 5, 7), 32, 96, 4), (BF16, 1, (4, 6, 10), 32, 96, 32),
    (BF16, 1, (3, 5, 7), 16, 48, 8), (F32, 1, (3, 5, 7), 16, 48, 32), (F32, 3, (3, 5, 7), 32, 32, 8), (BF16, 1, (3, 5, 7), 32, 32, 2),
]


def _a1_id(c):
    dtype, n, sp, c1, c2, G = c
    return f"{tn(dtype)}_N{n}_{'x'.join(map(str, sp))}_C{c1}{'+' + str(c2) if c2 else ''}_G{G}"


def _ppv(c, dtype):
    return c // (4 if dtype == F32 else 8)


@pytest.mark.parametrize("case", A1_CASES, ids=_a1_id)
def test_a1_gn_stats_full_pass_exact(case):
    ops = _ops()
    dtype, n, sp, c1, c2, G = case
    V, gs = math.prod(sp), (c1 + c2) // G
    xs = [ints((n,) + sp + (c,), 100 + k, terms=V * gs) for k, c in enumerate((c1, c2)) if c]
    ds = [dev(x, dtype) for x in xs] + [None]
    st = ops.gn_stats(ds[0], ds[1], G)
    assert_same_bits(st, ref_stats(xs, G), _a1_id(case))
    assert torch.equal(ops.gn_stats(ds[0], ds[1], G), st), "a repeated call gives other bits"


def test_a_case_tables_cover_the_issue():
    ppvs = {(_ppv(c, dt), 64 % _ppv(c, dt) == 0) for dt, n, sp, c1, c2, G in A1_CASES for c in (c1, c2) if c}
    assert {p for p, xor in ppvs if xor} == {1, 2, 4, 8, 16, 32, 64} and {p for p, xor in ppvs if not xor} >= {12, 20, 24, 48, 128}
    for dt in DTYPES:
        assert {c1 for d_, n, sp, c1, c2, G in A1_CASES if d_ == dt and not c2} >= ({96, 192, 512} if dt == F32 else {96, 160, 192, 384, 512})
    assert {G for *_, G in A1_CASES} >= {1, 2, 4, 8, 32, 64}
    sizes = {(c1 + c2) // G for dt, n, sp, c1, c2, G in A1_CASES}
    assert {1, 3, 512} <= sizes and min(sizes) == 1 and max(sizes) == 512
    assert {sp for _, _, sp, *_ in A1_CASES} >= {(3, 5, 7), (1, 1, 1), (48, 48, 48)} and {n for _, n, *_ in A1_CASES} == {1, 2, 3}
    for dt, n, sp, c1, c2, G in A1_CASES:
        if sp == (48, 48, 48):
            ppv = _ppv(c1, dt)
            bpn = B.blocks_per_sample(math.prod(sp) * ppv, ppv, n)
            assert -(-math.prod(sp) * ppv // (bpn * 256)) >= 8                  # every thread loops
    assert any(B.blocks_per_sample(math.prod(sp) * _ppv(c1, dt), _ppv(c1, dt), n) == 2048 // n for dt, n, sp, c1, c2, G in A1_CASES)
    halves = {(c1, c2) for dt, n, sp, c1, c2, G in A1_CASES if c2}
    assert halves == {(64, 32), (32, 96), (16, 48), (32, 32)}
    assert all({dt for dt, n, sp, c1, c2, G in A1_CASES if (c1, c2) == h} == set(DTYPES) for h in halves)
    # A2: all five conv kernel variants produce partials somewhere in the table; the fold paths of the hand-made partials
    L = _libmod().lib()
    seen = set()
    for case in GN_FUSED_CASES:
        name, N, (D, H, W), cin, cout, ks, stride, ups, circ = case
        for dt in DTYPES:
            conv = _ops().Conv(cin, cout, ks, stride=stride, upsample=ups, circular=circ)
            seen.add(L.vdm_conv_kernel_variant(conv.desc(N, D, H, W, dt), 0))
    assert seen == {0, 1, 2, 3, 4}, seen                                          # GENERIC, CLASS, KPACK, SPLIT, KSPLIT
    assert {c[0] for c in GN_FUSED_CASES} >= {"k3_ups", "k3_ups_circ", "k3_ups_ragged", "k3_ups_128_64", "k3_cin8_circ", "k3_deep_256_256"}
    assert {gs for gs, _ in A2_FOLD} == {12, 96, 128, 256} and all(t == [1, 7, 16 * (256 // gs) + 3] for gs, t in A2_FOLD)
    # B: the chain of the statistics stays at or below 64 additions (96 bf16 channels: 72, see B_CASES)
    for sp, c1, c2, G in B_CASES:
        for dt in DTYPES:
            dd = _b_chain(sp, c1, c2, G, dt)
            assert dd <= 64 or (dt == BF16 and c1 == 96 and dd == 72), (sp, c1, c2, G, dt, dd)
    assert {c1 + c2 for _, c1, c2, _ in B_CASES} == {16, 64, 96, 256} and {(c1, c2) for _, c1, c2, _ in B_CASES} >= {(32, 32), (64, 32), (96, 0)}
    assert {sp for sp, *_ in B_CASES} == {(3, 5, 7), (4, 6, 10), (16, 16, 16)} and {G for *_, G in B_CASES} >= {4, 8, 32}


# =============================================================================================== C: the workspace contract
def test_c_gn_stats_stays_inside_its_workspace():
    """n = 3, 32^3 voxels, 192 fp32 channels (48 pieces per voxel: the block count is a multiple of 3), 64 groups: the capped count
    682 used to be rounded UP to 684, 2052 rows of 128 floats - 2 KiB past VDM_GN_STATS_WS_BYTES.  The workspace here is followed by
    a 1 MiB guard of 0xA5 bytes inside the same allocation; it must come back untouched and the statistics exact."""
    ops, lm = _ops(), _libmod()
    n, sp, C, G = 3, (32, 32, 32), 192, 64
    V = math.prod(sp)
    x = ints((n,) + sp + (C,), 7, terms=V * (C // G))
    xd = x.to(DEV)
    ws = torch.full((lm.GN_STATS_WS_BYTES + (1 << 20),), 0xA5, dtype=torch.uint8, device=DEV)
    st = torch.zeros((n, G, 2), dtype=torch.float32, device=DEV)
    lm.check(lm.lib().vdm_gn_stats(xd.data_ptr(), C, None, 0, n, V, G, lm.VDM_F32, st.data_ptr(), ws.data_ptr(), None, 0, None, 0, None,
                                   torch.cuda.current_stream().cuda_stream), "vdm_gn_stats")
    torch.cuda.synchronize()
    guard = ws[lm.GN_STATS_WS_BYTES:]
    touched = (guard != 0xA5).nonzero()
    assert touched.numel() == 0, f"{touched.numel()} guard bytes behind the workspace were written, first at +{touched[0].item()}"
    assert_same_bits(st, ref_stats([x], G), "statistics of the capped pass")


def test_c_gn_stats_refuses_wide_groups_from_partials():
    """512 channels in one group from conv partials: refused, and stats / chsum stay as they were filled."""
    lm = _libmod()
    n, tiles, C = 2, 5, 512
    part = torch.ones((n, tiles, C, 2), dtype=torch.float32, device=DEV)
    x = torch.zeros((n, 4, C), dtype=BF16, device=DEV)
    st = torch.full((n, 1, 2), -7777.0, device=DEV)
    cs = torch.full((n, C), -7777.0, device=DEV)
    ws = torch.empty(lm.GN_STATS_WS_BYTES // 4, device=DEV)
    status = lm.lib().vdm_gn_stats(x.data_ptr(), C, None, 0, n, 4, 1, lm.VDM_BF16, st.data_ptr(), ws.data_ptr(), part.data_ptr(), tiles, None, 0,
                                   cs.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert status != 0 and b"channels per group" in lm.lib().vdm_last_error()
    assert bool((st == -7777.0).all()) and bool((cs == -7777.0).all()), "a refused call wrote its outputs"


# =============================================================================================== A2: statistics from conv partials
def selector_conv(case, dtype, seed):
    """A conv whose every output channel has ONE non-zero weight, +-1, at one (tap, input channel), with an integer bias and an integer
    residual: the output is a shifted, signed copy of an input channel plus small integers - exact in bf16 and fp32, tile sums exact.
    Returns (out with .gn_partials, the float64 reference of the conv or None where that would take too long)."""
    ops = _ops()
    name, N, (D, H, W), cin, cout, ks, stride, ups, circ = case
    ishape = (N, 2 * D, 2 * H, 2 * W, cin) if stride == 2 else (N, D // 2, H // 2, W // 2, cin) if ups else (N, D, H, W, cin)
    g = torch.Generator().manual_seed(seed)
    x = ints(ishape, seed + 1, terms=1)
    w = torch.zeros(ks ** 3, cout, cin)
    w[torch.randint(0, ks ** 3, (cout,), generator=g), torch.arange(cout), torch.randint(0, cin, (cout,), generator=g)] = \
        torch.randint(0, 2, (cout,), generator=g).float() * 2 - 1
    bias = ints((cout,), seed + 2, terms=1).clamp(-1, 1)
    res = ints((N, D, H, W, cout), seed + 3, terms=1).clamp(-1, 1)
    conv = ops.Conv(cin, cout, ks, stride=stride, upsample=ups, circular=circ)
    conv.pack(w.to(DEV), dtype, need_dgrad=False)
    xd = torch.zeros(ishape[:-1] + (ops.cpad(cin, dtype),), dtype=dtype, device=DEV)
    xd[..., :cin] = x.to(dtype).to(DEV)
    out = conv.fwd(xd, bias.to(DEV), None, dev(res, dtype), gn=True)
    ref = None
    if N * D * H * W * cin * cout * ks ** 3 <= 3e8:
        ref = ref_conv(x.double(), w.double(), bias.double(), None, res.double(), ks, stride, ups, circ)
    return out, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", GN_FUSED_CASES, ids=[c[0] for c in GN_FUSED_CASES])
def test_a2_gn_stats_from_conv_partials_exact(case, dtype):
    ops = _ops()
    G = 8
    out, ref = selector_conv(case, dtype, 300)
    name, N, sp, cin, cout = case[:5]
    assert out.gn_partials is not None and out.gn_partials.shape[0] == N and out.gn_partials.shape[2:] == (cout, 2)
    oc = out.float().cpu()
    if ref is not None:
        assert_same_bits(oc, ref, f"{name}: the selector conv itself")
    want = ref_stats([oc], G)
    assert_exact_sums(want)
    st = ops.gn_stats(out, None, G, chsum=True)
    assert_same_bits(st, want, f"{name}: statistics from the tile partials")
    assert_same_bits(st.chsum, oc.double().reshape(N, -1, cout).sum(1), f"{name}: per-channel sums")
    assert_same_bits(ops.gn_stats(out.clone(), None, G), want, f"{name}: full pass over the same tensor")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_a2_two_sources_from_partials_exact(dtype):
    """Both halves with partials and unequal widths: the single two-source launch (32 + 64 and 64 + 32 channels, 12 groups of 8);
    then one half with partials and the other read in full, in both orders."""
    ops = _ops()
    a, _ = selector_conv(next(c for c in GN_FUSED_CASES if c[0] == "k3_64_32"), dtype, 310)          # [1, 4, 8, 16, 32]
    b, _ = selector_conv(("k3_32_64", 1, (4, 8, 16), 32, 64, 3, 1, 0, False), dtype, 320)
    plain = ints((1, 4, 8, 16, 64), 330, terms=512 * 8)
    pd = dev(plain, dtype)
    assert a.gn_partials is not None and b.gn_partials is not None
    ac, bc = a.float().cpu(), b.float().cpu()
    for x1, x2, c1, c2 in ((a, b, ac, bc), (b, a, bc, ac)):
        st = ops.gn_stats(x1, x2, 12, chsum=True)
        assert_same_bits(st, ref_stats([c1, c2], 12), "two sources, one launch")
        assert_same_bits(st.chsum, torch.cat([c1, c2], -1).double().reshape(1, -1, 96).sum(1), "two sources: per-channel sums")
    for x1, x2, c1, c2 in ((a, pd, ac, plain), (pd, a, plain, ac)):
        st = ops.gn_stats(x1, x2, 12, chsum=True)
        assert st.chsum is None
        assert_same_bits(st, ref_stats([c1, c2], 12), "one half from partials, one read in full")


A2_FOLD = [(gs, [1, 7, 16 * (256 // gs) + 3]) for gs in (12, 96, 128, 256)]


@pytest.mark.parametrize("gs,tiles_list", A2_FOLD, ids=[f"gs{g}" for g, _ in A2_FOLD])
def test_a2_hand_made_partials_exact(gs, tiles_list):
    """tile_partials_fold's non-power-of-two and > 64 channels-per-group paths, one sweep, a ragged sweep and more than 16 sweeps."""
    ops = _ops()
    G = {12: 8, 96: 4, 128: 4, 256: 2}[gs]
    C, n = gs * G, 3
    for tiles in tiles_list:
        part = ints((n, tiles, C, 2), 400 + tiles, terms=tiles * gs)
        x = torch.zeros((n, 2, C), dtype=BF16, device=DEV)
        x.gn_partials = part.to(DEV)
        st = ops.gn_stats(x, None, G, chsum=True)
        assert_same_bits(st, part.double().sum(1).reshape(n, G, gs, 2).sum(2), f"gs {gs}, {tiles} tiles")
        assert_same_bits(st.chsum, part[..., 0].double().sum(1), f"gs {gs}, {tiles} tiles: per-channel sums")


# =============================================================================================== A3: channel sums
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 255, 257, 4099])
def test_a3_channel_sums_exact(rows, dtype):
    ops, lm = _ops(), _libmod()
    s = torch.cuda.current_stream().cuda_stream
    C = 40
    x = ints((rows, C), 500 + rows, terms=rows)
    buf, view, untouched = in_sentinel(C, (C,))
    lm.check(lm.lib().vdm_channel_sums(dev(x, dtype).data_ptr(), rows, C, ops.dt_id(dtype), view.data_ptr(), s), "vdm_channel_sums")
    torch.cuda.synchronize()
    assert untouched(), "channel_sums wrote outside its output"
    assert_same_bits(view, x.double().sum(0), f"channel_sums rows {rows}")
    n, c1, c2 = 3, 24, 8                                              # two sources of unequal widths
    a, b1, b2 = ints((n, rows, c1 + c2), 510 + rows, terms=rows), ints((n, rows, c1), 511 + rows, terms=rows), ints((n, rows, c2), 512 + rows, terms=rows)
    ad, b1d, b2d = dev(a, dtype), dev(b1, dtype), dev(b2, dtype)
    buf, view, untouched = in_sentinel(n * (c1 + c2) * 2, (n, 1, c1 + c2, 2))
    lm.check(lm.lib().vdm_channel_dot_sums(ad.data_ptr(), b1d.data_ptr(), c1, b2d.data_ptr(), c2, n, rows, ops.dt_id(dtype), view.data_ptr(), s),
             "vdm_channel_dot_sums")
    torch.cuda.synchronize()
    assert untouched(), "channel_dot_sums wrote outside its output"
    ref = torch.stack([a.double().sum(1), (a.double() * torch.cat([b1, b2], -1).double()).sum(1)], -1)[:, None]
    assert_same_bits(view, ref, f"channel_dot_sums rows {rows}")
    assert torch.equal(ops.channel_dot_sums(ad, b1d, b2d), view)


# =============================================================================================== A4: dbeta through finalize + apply
@pytest.mark.parametrize("case", [(F32, 3, (3, 5, 7), 32, 96, 4), (BF16, 3, (3, 5, 7), 16, 48, 8), (F32, 1, (4, 6, 10), 96, 0, 32),
                                  (BF16, 2, (4, 6, 10), 256, 0, 32), (BF16, 3, (3, 5, 7), 64, 32, 12)], ids=_a1_id)
def test_a4_dbeta_exact(case):
    """Integer dyh and integer gamma: dbeta = sum_n sum_v dyh and the per-sample sums never meet rstd - bit-equal to the int64 sums."""
    ops = _ops()
    dtype, n, sp, c1, c2, G = case
    C, V = c1 + c2, math.prod(sp)
    dyh = ints((n,) + sp + (C,), 600, terms=n * V)
    gamma = ints((C,), 601, terms=1)
    x = B.rnd64((n,) + sp + (C,), 602, dtype == BF16) + 0.5
    x1, x2 = dev(x[..., :c1], dtype), (dev(x[..., c1:], dtype) if c2 else None)
    st = ops.gn_stats(x1, x2, G)
    dd = dev(dyh, dtype)
    dd.gnb_partials = ops.channel_dot_sums(dd, x1, x2)
    assert_same_bits(dd.gnb_partials[:, 0, :, 0], dyh.double().reshape(n, V, C).sum(1), "per-sample channel sums of dyh")
    dgam, dbet = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    ops.gn_bwd_fused(x1, x2, G, st, gamma.to(DEV), dd, dgam, dbet, dx1=torch.empty_like(x1))
    assert_same_bits(dbet, dyh.double().reshape(-1, C).sum(0), "dbeta")
    assert torch.isfinite(dgam).all()


# =============================================================================================== A5: dropout bits
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_a5_dropout_bits_agree(dtype):
    """linear GroupNorm, n = 3, 105 voxels (not a multiple of any sweep): the zero pattern of the forward output, the keep-mask bytes
    and the zero pattern of the dyh that gn_silu_bwd's first launch (vdm_gn_dyh) forms for dy = 1 are the same bits.  Keep rate: the
    count is binomial(M, 1 - p); 5 standard deviations (+ 8e-6: the 16-bit threshold of bf16 storage)."""
    ops, lm = _ops(), _libmod()
    n, sp, C, G, p, seed = 3, (3, 5, 7), 32, 8, 0.25, 4242
    V, epl = math.prod(sp), ops.epl(dtype)
    x = dev(B.rnd64((n,) + sp + (C,), 700, dtype == BF16) + 0.3, dtype)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    st = ops.gn_stats(x, None, G)
    y0 = ops.gn_silu_fwd(x, None, G, st, gamma, beta, linear=True)
    assert bool((y0 != 0).all()), "a normalised value is 0: the zero pattern would not be the dropout mask"
    y = ops.gn_silu_fwd(x, None, G, st, gamma, beta, p, seed, want_mask=True, linear=True)
    kept = (y != 0).reshape(n, V, C)
    bits = ((y.keep_mask.to(torch.int32)[..., None] >> torch.arange(epl, device=DEV)) & 1).reshape(n, V, C).bool()
    assert y.keep_mask.shape == (n, V, C // epl) and torch.equal(kept, bits), "mask bytes differ from the zeros of the forward output"
    assert torch.equal(ops.gn_silu_fwd(x, None, G, st, gamma, beta, p, seed, linear=True), y)          # without the mask output: same bits
    dy, dyh = torch.ones_like(x), torch.empty_like(x)
    lm.check(lm.lib().vdm_gn_dyh(x.data_ptr(), C, None, 0, n, V, G, ops.dt_id(dtype), st.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ops.GN_EPS,
                                 p, seed, dy.data_ptr(), dyh.data_ptr(), 1, None, torch.cuda.current_stream().cuda_stream), "vdm_gn_dyh")
    assert torch.equal((dyh != 0).reshape(n, V, C), kept), "the backward regenerates other keep bits"
    scale = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32).to(dtype).float().item()
    assert bool((dyh[dyh != 0].float() == scale).all())
    if dtype == F32:                      # (bf16: y0 is the rounded value, the kept ones are scaled before their own rounding)
        assert torch.equal(y[y != 0], (y0 * torch.tensor(1.0 / (1.0 - p), dtype=F32, device=DEV))[y != 0])
    M = n * V * C
    rate = kept.float().mean().item()
    assert abs(rate - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / M) + 8e-6, rate


# =============================================================================================== B: random reals against float64
# voxel shape, c1, c2, groups (n = 2).  d = the chain of the statistics (fp32 / bf16 storage), asserted in the table test:
#   (3,5,7) 16 G4: 24 / 24    (4,6,10) 32+32 G8: 45 / 42    (4,6,10) 64+32 G12: 45 / 45    (3,5,7) 96 G32: 41 / 72    (4,6,10) 256 G32: 46 / 46
#   16^3 16 G8: 29 / 26.  96 bf16 channels are 12 pieces per voxel: the generic path parks 256 thread sums and one thread walks the 22
#   of its piece column times the 3 channels of a group, 66 additions - no group count of {4, 8, 32} brings that width below 64.
B_CASES = [((3, 5, 7), 16, 0, 4), ((4, 6, 10), 32, 32, 8), ((4, 6, 10), 64, 32, 12), ((3, 5, 7), 96, 0, 32), ((4, 6, 10), 256, 0, 32),
           ((16, 16, 16), 16, 0, 8)]
KINDS = B.OFFSETS + B.SPECIAL
D_TILE = 8 + 4 + 3          # a conv epilogue's tile sums: NV <= 8 rows per lane, four DPP steps, the fold over the waves


def _b_chain(sp, c1, c2, G, dtype):
    epl, gs = (4 if dtype == F32 else 8), (c1 + c2) // G
    return max(B.stats_chain(c, math.prod(sp), 2, epl, gs) for c in (c1, c2) if c)


class Worst(dict):
    def take(self, name, got, ref, bound, what):
        got = got.detach().double().cpu().reshape(ref.shape)
        err = (got - ref).abs()
        assert torch.isfinite(got).all() and torch.isfinite(bound).all(), f"{what}: {name} not finite"
        ratio = (err / bound.clamp_min(1e-300)).max().item() if err.max().item() > 0 else 0.0
        self[name] = max(self.get(name, 0.0), ratio)
        print(f"GN B {what} {name}: max err {err.max().item():.3e} err/bound {ratio:.4f}")
        assert (err <= bound).all(), f"{what}: {name} err / bound {ratio:.3f} at {(err / bound.clamp_min(1e-300)).argmax().item()}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS, ids=[str(k) for k in KINDS])
def test_b_every_consumer_against_float64(kind, dtype):
    ops = _ops()
    bf16 = dtype == BF16
    worst, ran = Worst(), set()
    for ci, (sp, c1, c2, G) in enumerate(B_CASES):
        N, V, C = 2, math.prod(sp), c1 + c2
        gs = C // G
        what = f"{kind} {tn(dtype)} {'x'.join(map(str, sp))} C{c1}+{c2} G{G}"
        d, d1 = _b_chain(sp, c1, c2, G, dtype), B.dot_sums_chain(V)
        x = B.gn_input(kind, N, V, C, G, 800 + ci, bf16)
        gamma, beta = (1.0 + 0.3 * B.rnd64((C,), 801, False)).float().double(), (0.2 * B.rnd64((C,), 802, False)).float().double()
        dy, add = B.rnd64((N, V, C), 803, bf16), B.rnd64((N, V, C), 804, bf16)
        full = lambda t: t.reshape((N,) + sp + (t.shape[-1],))
        x1, x2 = dev(full(x[..., :c1]), dtype), (dev(full(x[..., c1:]), dtype) if c2 else None)
        gd, bd = gamma.float().to(DEV), beta.float().to(DEV)
        st = ops.gn_stats(x1, x2, G)
        # ---- gn_silu_fwd, SiLU and linear
        fw = {}
        for linear in (False, True):
            fw[linear] = B.fwd(x, gamma, beta, G, d, linear, bf16)
            y = ops.gn_silu_fwd(x1, x2, G, st, gd, bd, linear=linear)
            worst.take("fwd_linear" if linear else "fwd_silu", y, fw[linear].y, fw[linear].bound, what)
        y_silu = ops.gn_silu_fwd(x1, x2, G, st, gd, bd)
        # ---- gn_silu_bwd = gn_dyh + channel_dot_sums + finalize + apply, with add1 / add2 and colsum
        a1, a2 = dev(full(add[..., :c1]), dtype), (dev(full(add[..., c1:]), dtype) if c2 else None)
        for linear in (False, True):
            ref_dyh, b_dyh = B.dyh_stage(fw[linear], dy, linear, bf16)
            bw = B.bwd(x, ref_dyh, gamma, G, d, d1, bf16, dyh_err=b_dyh, add=add)
            dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            cs = torch.zeros(N, C + 5, device=DEV)
            st.chsum = None
            dx1, dx2 = ops.gn_silu_bwd(x1, x2, G, st, gd, bd, dev(full(dy), dtype), dgam, dbet, add1=a1, add2=a2, colsum=cs[:, 2:2 + C],
                                       linear=linear)
            dx = dx1 if dx2 is None else torch.cat([dx1, dx2], -1)
            tag = "bwd_linear" if linear else "bwd_silu"
            worst.take(tag + "_dx", dx, bw.dx, bw.b_dx, what)
            worst.take(tag + "_dgamma", dgam, bw.dgamma, bw.b_dgamma, what)
            worst.take(tag + "_dbeta", dbet, bw.dbeta, bw.b_dbeta, what)
            worst.take(tag + "_colsum", cs[:, 2:2 + C], bw.colsum, bw.b_colsum, what)
            assert cs[:, :2].abs().max().item() == 0 and cs[:, 2 + C:].abs().max().item() == 0
        st.chsum = None
        # ---- the skip-fused passes (bf16 storage, the channel splits csrc/gn_skip.hip serves)
        cout = {16: 32, 64: 32}.get(C, 32)
        fwd_ok, bwd_ok = ops.gn_skip_supported(c1, c2, cout, dtype)
        if fwd_ok:
            w = B.rnd64((cout, C), 810, False, scale=C ** -0.5).float()
            w1, w2 = w[:, :c1].contiguous().to(DEV), (w[:, c1:].contiguous().to(DEV) if c2 else None)
            ys, _ = ops.gn_silu_skip_fwd(x1, x2, G, st, gd, bd, w1, w2, torch.zeros(cout, device=DEV))
            assert torch.equal(ys, y_silu), f"{what}: the skip-fused forward's activation differs from gn_silu_fwd's"
            ran.add("skip_fwd")
            if bwd_ok:
                dyh_s, dout = B.rnd64((N, V, C), 811, True), B.rnd64((N, V, cout), 812, True)
                wb = w.bfloat16().double()
                extra = (dout @ wb, (cout + 2) * B.U * (dout.abs() @ wb.abs()))
                bw = B.bwd(x, dyh_s, gamma, G, d, d1, True, extra_dx=extra)
                dd, ddout = dev(full(dyh_s), dtype), dev(full(dout), dtype)
                dd.gnb_partials = ops.channel_dot_sums(dd, x1, x2)
                dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
                dw1, dw2 = torch.zeros(cout, c1, device=DEV), (torch.zeros(cout, c2, device=DEV) if c2 else None)
                dx1, dx2 = ops.gn_bwd_fused(x1, x2, G, st, gd, dd, dgam, dbet, skip=(ddout, w1, w2, dw1, dw2))
                dx = dx1 if dx2 is None else torch.cat([dx1, dx2], -1)
                worst.take("skip_bwd_dx", dx, bw.dx, bw.b_dx, what)
                worst.take("skip_bwd_dgamma", dgam, bw.dgamma, bw.b_dgamma, what)
                worst.take("skip_bwd_dbeta", dbet, bw.dbeta, bw.b_dbeta, what)
                ran.add("skip_bwd")
        if c2 == 0 and bf16:
            # ---- gn_bwd_fused(tail=...): equals the apply pass + conv_in's weight gradient bit for bit
            conv_in = ops.Conv(2, C, 3)
            if ops.gn_tail_ok(conv_in, x1):
                xin = dev(torch.cat([B.rnd64((N,) + sp + (2,), 830, True), torch.zeros((N,) + sp + (6,), dtype=torch.float64)], -1), dtype)
                dd = dev(full(dy), dtype)
                part = ops.channel_dot_sums(dd, x1, None)
                outs = []
                for fused in (False, True):
                    t = dd.clone()
                    t.gnb_partials = part
                    dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
                    dw, db = torch.zeros(27, C, 2, device=DEV), torch.zeros(C, device=DEV)
                    if fused:
                        ops.gn_bwd_fused(x1, None, G, st, gd, t, dgam, dbet, add1=a1, tail=(conv_in, xin, dw, db))
                    else:
                        dxr, _ = ops.gn_bwd_fused(x1, None, G, st, gd, t, dgam, dbet, add1=a1)
                        conv_in.wgrad(xin, dxr, dw, db)
                    outs.append((dw, db, dgam, dbet))
                assert all(torch.equal(p, q) for p, q in zip(*outs)), f"{what}: the wgrad_thin tail differs from apply + wgrad"
                ran.add("tail")
        # ---- Conv.dgrad_gn + gn_bwd_fused
        conv = ops.Conv(C, 32, 3)
        if conv.gn_fold_ok(c1, c2, dtype):
            wc = B.rnd64((27, 32, C), 840, bf16, scale=(27 * C) ** -0.5)
            conv.pack(wc.float().to(DEV), dtype, need_dgrad=True)
            dout = B.rnd64((N,) + sp + (32,), 841, bf16)
            dd = dev(dout, dtype)
            dyh_f = conv.dgrad_gn(dd, x1, x2, G, st, gd, bd)
            g_plain = conv.dgrad(dd).double().cpu().reshape(N, V, C)
            cabs = ops.Conv(C, 32, 3)
            cabs.pack(wc.abs().float().to(DEV), dtype, need_dgrad=True)
            S = cabs.dgrad(dev(dout.abs(), dtype)).double().cpu().reshape(N, V, C) * (1 + 2 * B.UB)
            f = fw[False]
            sp_ = B.dsilu(f.ylin)
            ref = g_plain * sp_
            # two accumulation orders of the same 27 * 32 products (fp32 storage: three bf16 products each), the plain result's storage rounding
            e_g = 2 * (27 * 32 * (1 if bf16 else 3) + 1) * B.U * S + (B.UB * g_plain.abs() * (1 + B.UB) if bf16 else 0.0)
            bnd = g_plain.abs() * (B.DSILU_LIP * f.dylin + B.dsilu_eval_err(f.ylin)) + e_g * (sp_.abs() + B.DSILU_LIP * f.dylin) + B.U * ref.abs()
            worst.take("dgrad_gn_dyh", dyh_f, ref, B.store_err(ref, bnd, bf16), what)
            tiles = dyh_f.gnb_partials.shape[1]
            dyh_st = dyh_f.double().cpu().reshape(N, V, C)
            st.chsum = torch.cat([ops.channel_dot_sums(t, t)[:, 0, :, 0] for t in (x1, x2) if t is not None], 1).contiguous()
            bw = B.bwd(x, dyh_st, gamma, G, d, D_TILE + B.fold_chain(tiles, gs), bf16, add=add, pre_round=B.UB if bf16 else 0.0, chsum_chain=d1)
            dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            cs = torch.zeros(N, C, device=DEV)
            dx1, dx2 = ops.gn_bwd_fused(x1, x2, G, st, gd, dyh_f, dgam, dbet, add1=a1, add2=a2, colsum=cs, dx1=torch.empty_like(x1))
            dx = dx1 if dx2 is None else torch.cat([dx1, dx2], -1)
            worst.take("fold_dx", dx, bw.dx, bw.b_dx, what)
            worst.take("fold_dgamma", dgam, bw.dgamma, bw.b_dgamma, what)
            worst.take("fold_dbeta", dbet, bw.dbeta, bw.b_dbeta, what)
            worst.take("fold_colsum", cs, bw.colsum_gn, bw.b_colsum_gn, what)          # (gn_bwd_fused's colsum: the GroupNorm part alone)
            st.chsum = None
            ran.add("fold")
    assert "fold" in ran and (not bf16 or ran >= {"skip_fwd", "skip_bwd", "tail", "fold"}), ran
    print(f"GN B SUMMARY {kind} {tn(dtype)}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
