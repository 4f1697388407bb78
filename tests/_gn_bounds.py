"""Float64 references and derived fp32 error bounds of the GroupNorm kernels (the derivation stands in the docstring of
tests/test_groupnorm_kernels_gpu.py; tests/test_groupnorm_cpu.py holds a plain torch-fp32 evaluation of the same raw-moment formulas
against every bound here).  Everything is torch float64 on the CPU; tensors are [N, V, C] (voxels flattened), per-group quantities
[N, G], per-channel ones [N, G, gs].  Nothing in this file is fitted to a kernel's output."""
import math
from types import SimpleNamespace as NS

import torch

U = 2.0 ** -24                 # unit roundoff of fp32
UB = 2.0 ** -8                 # unit roundoff of bf16 storage (8 significant bits, round to nearest even)
EPS = 1e-5                     # GN_EPS of the product
SILU_LIP = 1.1                 # sup |silu'| = 1.0998...
DSILU_LIP = 0.5                # sup |silu''| = 0.5


# ------------------------------------------------------------------------------------------ chain lengths, counted from the code
def blocks_per_sample(npieces, ppv, n):
    """csrc/elementwise.hip stats_blocks_per_sample (workgroups per sample of the full statistics pass)."""
    want = max(1, min((npieces + 2047) // 2048, max(2048 // n, 1)))
    m = ppv // math.gcd(ppv, 256)
    want = (want + m - 1) // m * m
    if want > max(2048 // n, 1):
        want = max(2048 // n, 1) // m * m
    return max(want, m)


def stats_chain(c_src, voxels, n, epl, gs):
    """Longest chain of fp32 additions one element's contribution passes through in vdm_gn_stats' full pass over a source of c_src
    channels (gn_stats_kernel + gn_stats_finalize_kernel): the thread's sweep, the xor-butterfly, the LDS fold, the two finalize folds.
    Additions of an exact zero (idle finalize parts) are not counted: they round nothing."""
    ppv = c_src // epl
    bpn = blocks_per_sample(voxels * ppv, ppv, n)
    sweep = -(-voxels * ppv // (bpn * 256))
    if 64 % ppv == 0:
        fly, fold = int(math.log2(64 // ppv)), 4 * gs
    else:
        fly, fold = 0, (256 // ppv + 1) * min(gs, c_src)
    gc = c_src // gs
    parts = max(256 // (2 * gc), 1)
    return sweep + fly + fold + -(-bpn // parts) + min(parts, bpn)


def dot_sums_chain(voxels):
    """vdm_channel_dot_sums / vdm_channel_sums: rows / 256 per thread, six butterfly steps, three adds over the four waves."""
    return -(-voxels // 256) + 6 + 3


def fold_chain(tiles, gs):
    """tile_partials_fold<256> of csrc/elementwise.hip: tiles / per sequential loads per thread, then the butterfly and the four waves
    (power-of-two gs <= 64) or the walk over the `per` parked sums."""
    per = 256 // gs
    seq = -(-tiles // per)
    if gs <= 64 and gs & (gs - 1) == 0:
        return seq + int(math.log2(64 // gs)) + 4
    return seq + per


# ------------------------------------------------------------------------------------------ float64 reference quantities
def sigmoid(y):
    return torch.sigmoid(y)


def silu(y):
    return y * torch.sigmoid(y)


def dsilu(y):
    s = torch.sigmoid(y)
    return s * (1.0 + y * (1.0 - s))


def moments(x, G):
    """x [N, V, C] float64 -> the float64 group quantities of the derivation: m, q, v (two-pass, what F.group_norm computes), rho, a1."""
    N, V, C = x.shape
    gs = C // G
    xg = x.reshape(N, V, G, gs)
    cnt = V * gs
    m = xg.sum((1, 3)) / cnt
    q = (xg * xg).sum((1, 3)) / cnt
    a1 = xg.abs().sum((1, 3)) / cnt
    v = ((xg - m[:, None, :, None]) ** 2).sum((1, 3)) / cnt
    return NS(N=N, V=V, C=C, G=G, gs=gs, cnt=cnt, xg=xg, m=m, q=q, a1=a1, v=v, rho=(v + EPS) ** -0.5)


def stat_err(M, d):
    """|dm|, Ev, rho* and |drho| of the raw-moment statistics after chains of d additions (see the derivation)."""
    dm = (d + 1) * U * M.a1
    Ev = (d + 2) * U * M.q + 2 * M.m.abs() * dm + 2 * U * M.m ** 2 + U * M.v
    rs = ((M.v - Ev).clamp_min(0.0) + EPS) ** -0.5
    drho = 0.5 * rs ** 3 * Ev + 4 * U * rs
    return NS(dm=dm, Ev=Ev, rs=rs, drho=drho)


def _g(t):          # [N, G] -> broadcast over [N, V, G, gs]
    return t[:, None, :, None]


def _c(t, G):       # [C] -> [1, 1, G, gs]
    return t.reshape(1, 1, G, -1)


def silu_eval_err(y, dy):
    """Evaluation error of the device silu(y) = y * rcp(1 + __expf(-y)) at an argument within dy of y: __expf(-y) = exp2(-y log2 e) has a
    relative error of 2u (|y| + 2) (the rounded product in the exponent, one ulp of v_exp_f32), which reaches sigma as (1 - sigma) of
    that; the addition (u), v_rcp_f32 (one ulp = 2u) and the product (u) follow:  u |silu| (4 + 2 (1 - sigma)(|y| + 2)) <=
    u |silu| (8 + 2 (1 - sigma) |y|)."""
    s = torch.sigmoid(y)
    return U * (silu(y).abs() + SILU_LIP * dy) * (8.0 + 2.0 * (1.0 - s) * (y.abs() + dy))


def dsilu_eval_err(y):
    """Evaluation error of the device silu'(y) = s (1 + y (1 - s)), s = 1 / (1 + __expf(-y)):  ds <= s u (2 (1 - s)(|y| + 2) + 2) (the
    exponential, the addition, the division) enters through d silu' / d s = 1 + y - 2 y s, |.| <= 1 + |y|; the roundings of 1 - s,
    y (1 - s), 1 + . and the last product add s u (2 |y| + 2) + u |silu'|."""
    s = torch.sigmoid(y)
    ay = y.abs()
    return U * ((1.0 + ay) * s * (2.0 * (1.0 - s) * (ay + 2.0) + 2.0) + s * (2.0 * ay + 2.0) + dsilu(y).abs())


def store_err(ref, b, bf16):
    """The stored value: fp32 keeps the computed one, bf16 rounds it to nearest (2^-8 relative of the computed value)."""
    return b + UB * (ref.abs() + b) if bf16 else b


# ------------------------------------------------------------------------------------------ forward
def fwd(x, gamma, beta, G, d, linear, bf16):
    """Reference y = silu(groupnorm(x)) (linear: groupnorm(x)) in float64 and the bound of the kernels' y, both [N, V, C]."""
    M = moments(x, G)
    S = stat_err(M, d)
    gam, bet = _c(gamma, G), _c(beta, G)
    xc = M.xg - _g(M.m)
    ylin = xc * _g(M.rho) * gam + bet
    rs = _g(S.rs)
    dylin = gam.abs() * (xc.abs() * _g(S.drho) + rs * _g(S.dm)) + 4 * U * ((M.xg * gam * rs).abs() + (_g(M.m) * gam * rs).abs() + bet.abs())
    if linear:
        y, b = ylin, dylin
    else:
        y, b = silu(ylin), SILU_LIP * dylin + silu_eval_err(ylin, dylin)
    shp = (M.N, M.V, M.C)
    return NS(M=M, S=S, y=y.reshape(shp), bound=store_err(y, b, bf16).reshape(shp), ylin=ylin.reshape(shp), dylin=dylin.reshape(shp))


def dyh_stage(F, dy, linear, bf16):
    """gn_dyh: dyh = dy silu'(ylin) stored in the storage type (linear: dyh = dy, exact).  F = fwd(...).  Returns (ref, bound)."""
    if linear:
        return dy, torch.zeros_like(dy)
    ref = dy * dsilu(F.ylin)
    b = dy.abs() * (DSILU_LIP * F.dylin + dsilu_eval_err(F.ylin)) + U * ref.abs()
    return ref, store_err(ref, b, bf16)


# ------------------------------------------------------------------------------------------ backward: finalize + apply
def bwd(x, dyh, gamma, G, d, d1, bf16, dyh_err=None, add=None, pre_round=0.0, chsum_chain=None, extra_dx=None):
    """GroupNorm backward behind dyh (the gradient at the GroupNorm output, [N, V, C]):  dx = rho (gamma dyh - m1 - xhat m2) (+ add),
    dgamma, dbeta, colsum = sum_v dx in float64, and their bounds.
      d        chain of the forward statistics, d1 the chain of the per-channel sums T1 = sum_v dyh, T2 = sum_v dyh x
      dyh_err  elementwise bound of |device dyh - dyh| (None: dyh holds the device's own stored values, exact)
      pre_round  relative error of the summed values against the stored dyh (a conv epilogue sums its fp32 results before the bf16
                 rounding: 2^-8; 0 where the sums are taken from the stored tensor)
      extra_dx (ref, bound): a further fp32 term added to dx before the store (the skip conv's W^T dout)"""
    M = moments(x, G)
    S = stat_err(M, d)
    N, V, gs, cnt = M.N, M.V, M.gs, M.cnt
    gam = gamma.reshape(1, G, gs)
    dg = dyh.reshape(N, V, G, gs)
    de = torch.zeros_like(dg) if dyh_err is None else dyh_err.reshape(N, V, G, gs)
    m, rho, dm, drho, rs = (t[:, :, None] for t in (M.m, M.rho, S.dm, S.drho, S.rs))          # [N, G, 1]
    xc = M.xg - _g(M.m)
    xh = xc * _g(M.rho)
    T1, T2r, Tx = dg.sum(1), (dg * M.xg).sum(1), (dg * xh).sum(1)                                # [N, G, gs]
    A1, A2 = dg.abs().sum(1), (dg * M.xg).abs().sum(1)
    e1 = (d1 * U + pre_round) * A1 + de.sum(1)
    e2 = ((d1 + 1) * U + pre_round) * A2 + (de * M.xg.abs()).sum(1)
    D = (dg * xc).sum(1)                                                                         # T2r - m T1, without the cancellation
    ex = drho * D.abs() + rs * (e2 + m.abs() * e1 + dm * T1.abs() + U * (m * T1).abs() + U * D.abs()) + U * Tx.abs()
    dbeta, e_dbeta = T1.sum(0), e1.sum(0) + (N - 1) * U * T1.abs().sum(0)
    dgamma, e_dgamma = Tx.sum(0), ex.sum(0) + (N - 1) * U * Tx.abs().sum(0)
    r1, r2 = (gam * T1).sum(-1, keepdim=True), (gam * Tx).sum(-1, keepdim=True)                  # [N, G, 1]
    er1 = (gam.abs() * e1).sum(-1, keepdim=True) + (gs + 1) * U * (gam * T1).abs().sum(-1, keepdim=True)
    er2 = (gam.abs() * ex).sum(-1, keepdim=True) + (gs + 1) * U * (gam * Tx).abs().sum(-1, keepdim=True)
    m1, m2 = r1 / cnt, r2 / cnt
    dm1, dm2 = er1 / cnt + U * m1.abs(), er2 / cnt + U * m2.abs()
    b = lambda t: t[:, None]                                                                     # [N, G, 1] -> [N, 1, G, 1]
    gam4 = gam[:, None]
    dx = b(rho) * (gam4 * dg - b(m1) - xh * b(m2))
    Q, R = -b(rho) ** 2 * b(m2), b(rho) * (b(m) * b(rho) * b(m2) - b(m1))
    bdx = (b(drho) * (gam4 * dg - b(m1) - 2 * xh * b(m2)).abs() + b(rs) ** 2 * b(m2).abs() * b(dm) + b(rs) * b(dm1)
           + b(rs) * xc.abs() * b(rs) * b(dm2) + b(rs) * gam4.abs() * de
           + U * (2 * (gam4 * b(rs) * dg).abs() + 2 * b(rs) ** 2 * (b(m2) * M.xg).abs() + 3 * b(rs) ** 2 * (b(m) * b(m2)).abs()
                  + b(rs) * (b(m) * b(rho) * b(m2) - b(m1)).abs() + R.abs() + (M.xg * Q + R).abs() + dx.abs()))
    shp = (N, V, M.C)
    dx, bdx = dx.reshape(shp), bdx.reshape(shp)
    if extra_dx is not None:
        dx, bdx = dx + extra_dx[0], bdx + extra_dx[1] + U * (dx + extra_dx[0]).abs()
    # analytic column sums: colsum = rho (gamma T1 - V m1 - m2 xhsum), xhsum = rho (chsum - V mean)
    dch = d1 if chsum_chain is None else chsum_chain
    chs = M.xg.sum(1)
    e_ch = dch * U * M.xg.abs().sum(1)
    Dc = xc.sum(1)                                                                               # chsum - V m
    xhs = rho * Dc
    e_xhs = drho * Dc.abs() + rs * (e_ch + V * dm + U * V * m.abs() + U * Dc.abs()) + U * xhs.abs()
    inner = gam * T1 - V * m1 - m2 * xhs
    cs = rho * inner
    e_cs = (drho * inner.abs() + rs * (gam.abs() * e1 + V * dm1 + dm2 * xhs.abs() + m2.abs() * e_xhs
                                       + 3 * U * ((gam * T1).abs() + V * m1.abs() + (m2 * xhs).abs())) + U * cs.abs())
    cs, e_cs = cs.reshape(N, M.C), e_cs.reshape(N, M.C)
    cs_gn, e_cs_gn = cs, e_cs
    if add is not None:
        dx, bdx = dx + add, bdx + U * (dx + add).abs()
        cs, e_cs = cs + add.sum(1), e_cs + dot_sums_chain(V) * U * add.abs().sum(1) + U * (cs + add.sum(1)).abs()
    return NS(dx=dx, b_dx=store_err(dx, bdx, bf16), dgamma=dgamma.reshape(-1), b_dgamma=e_dgamma.reshape(-1), dbeta=dbeta.reshape(-1),
              b_dbeta=e_dbeta.reshape(-1), colsum=cs, b_colsum=e_cs, colsum_gn=cs_gn, b_colsum_gn=e_cs_gn, M=M, S=S)


# ------------------------------------------------------------------------------------------ the same formulas in plain torch fp32
def f32_stats(x, G):
    """{sum, sumsq} per (sample, group) of x [N, V, C] in fp32 (torch's pairwise sums: a chain of about log2 of the count)."""
    N, V, C = x.shape
    xg = x.float().reshape(N, V, G, C // G).permute(0, 2, 1, 3).reshape(N, G, -1).contiguous()
    return torch.stack([xg.sum(-1), (xg * xg).sum(-1)], -1)


def f32_affine(stats, cnt):
    """mean and rstd as gn_affine of csrc/elementwise.hip forms them, every operation in fp32."""
    cnt = torch.tensor(float(cnt), dtype=torch.float32)
    mean = stats[..., 0] / cnt
    var = (stats[..., 1] / cnt - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + torch.tensor(EPS, dtype=torch.float32))


def f32_fwd(x, gamma, beta, G, linear, bf16):
    N, V, C = x.shape
    gs = C // G
    mean, rstd = f32_affine(f32_stats(x, G), V * gs)
    A = rstd[:, :, None] * gamma.float().reshape(1, G, gs)
    B = beta.float().reshape(1, G, gs) - mean[:, :, None] * A
    y = x.float().reshape(N, V, G, gs) * A[:, None] + B[:, None]
    if not linear:
        y = y * (1.0 / (1.0 + torch.exp(-y)))
    y = y.reshape(N, V, C)
    return y.bfloat16().float() if bf16 else y


def f32_dyh(x, dy, gamma, beta, G, linear, bf16):
    if linear:
        return dy.float()
    N, V, C = x.shape
    gs = C // G
    mean, rstd = f32_affine(f32_stats(x, G), V * gs)
    A = rstd[:, :, None] * gamma.float().reshape(1, G, gs)
    B = beta.float().reshape(1, G, gs) - mean[:, :, None] * A
    y = x.float().reshape(N, V, G, gs) * A[:, None] + B[:, None]
    s = 1.0 / (1.0 + torch.exp(-y))
    d = (dy.float().reshape(N, V, G, gs) * (s * (1.0 + y * (1.0 - s)))).reshape(N, V, C)
    return d.bfloat16().float() if bf16 else d


def f32_bwd(x, dyh, gamma, G, bf16, add=None):
    """gn_bwd_finalize_kernel + gn_bwd_apply_kernel in torch fp32: returns (dx, dgamma, dbeta, colsum)."""
    N, V, C = x.shape
    gs = C // G
    f = torch.float32
    xs, ds, gam = x.float().reshape(N, V, G, gs), dyh.float().reshape(N, V, G, gs), gamma.float().reshape(1, G, gs)
    cnt = torch.tensor(float(V * gs), dtype=f)
    mean, rstd = f32_affine(f32_stats(x, G), V * gs)
    mean, rstd = mean[:, :, None], rstd[:, :, None]
    vsum = lambda t: t.permute(0, 2, 3, 1).contiguous().sum(-1)          # over the voxels, contiguous: torch's pairwise sum
    T1, T2 = vsum(ds), vsum(ds * xs)
    T2 = rstd * (T2 - mean * T1)
    r1, r2 = (gam * T1).sum(-1, keepdim=True), (gam * T2).sum(-1, keepdim=True)
    m1, m2 = r1 / cnt, r2 / cnt
    P, Q, R = rstd * gam, -rstd * rstd * m2, rstd * (mean * rstd * m2 - m1)
    dx = (ds * P[:, None] + (xs * Q[:, None] + R[:, None])).reshape(N, V, C)
    Vf = torch.tensor(float(V), dtype=f)
    xhsum = rstd * (vsum(xs) - Vf * mean)
    cs = (rstd * (gam * T1 - Vf * m1 - m2 * xhsum)).reshape(N, C)
    if add is not None:
        dx = dx + add.float()
        cs = cs + add.float().permute(0, 2, 1).contiguous().sum(-1)
    return (dx.bfloat16().float() if bf16 else dx), T2.sum(0).reshape(-1), T1.sum(0).reshape(-1), cs


# ------------------------------------------------------------------------------------------ inputs of the conditioning cases
OFFSETS = [0, 1, 4, 16, 64]
SPECIAL = ["const_group", "tiny_std", "mixed_offsets"]


def gn_input(kind, N, V, C, G, seed, bf16):
    """GroupNorm inputs mean + std randn rounded to the storage type, as float64 [N, V, C]: kind = |mean| / std of every group (a
    number), or "const_group" (group 0 constant, std 0), "tiny_std" (group 0: std 0.01 around 0), "mixed_offsets" (group g carries
    the offset OFFSETS[g % 5] with alternating sign)."""
    g = torch.Generator().manual_seed(seed)
    gs = C // G
    x = torch.randn(N, V, G, gs, generator=g)
    if kind == "const_group":
        x[:, :, 0, :] = 1.75
    elif kind == "tiny_std":
        x[:, :, 0, :] *= 0.01
    elif kind == "mixed_offsets":
        x = x + torch.tensor([OFFSETS[i % 5] * (-1.0) ** i for i in range(G)]).reshape(1, 1, G, 1)
    else:
        x = x + float(kind)
    x = x.reshape(N, V, C)
    return (x.bfloat16() if bf16 else x).double()


def rnd64(shape, seed, bf16, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * scale
    return (x.bfloat16() if bf16 else x).double()
