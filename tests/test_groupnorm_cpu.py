"""CPU side of the GroupNorm kernel tests (tests/test_groupnorm_kernels_gpu.py):
  * the float64 formulas of tests/_gn_bounds.py ARE F.group_norm / F.silu and their autograd in float64;
  * a plain torch-fp32 evaluation of the raw-moment formulas the kernels use (sum / cnt, sumsq / cnt - mean^2, rsqrt, the P / Q / R
    form of the backward) stays inside every derived bound, at every conditioning case - the bounds hold for the formulation itself,
    not for one device;
  * the bounds are sharp enough to notice a wrong formula: at |mean| / std = 0 they reject a reference evaluated without eps on a
    group of std 0.01 (a 4.9 % change of rstd);
  * the two refusals of vdm_gn_stats (host only: nothing is launched, the pointers are never followed)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _gn_bounds as B

KINDS = B.OFFSETS + B.SPECIAL
SHAPES = [(2, 105, 16, 4), (2, 240, 96, 32), (2, 240, 64, 8), (2, 4096, 16, 8), (2, 240, 256, 32)]      # N, V, C, G
D_CPU = 16          # torch's CPU sums are pairwise: a chain of about log2(count) additions, 16 covers 2^16 elements per group
PTR = ctypes.c_void_p(4096)
ERR_ARG = -1


def _case(kind, shape, bf16, seed=0):
    N, V, C, G = shape
    x = B.gn_input(kind, N, V, C, G, 100 + seed, bf16)
    gamma, beta = 1.0 + 0.3 * B.rnd64((C,), 101, False), 0.2 * B.rnd64((C,), 102, False)
    gamma, beta = gamma.float().double(), beta.float().double()
    dy, add = B.rnd64((N, V, C), 103, bf16), B.rnd64((N, V, C), 104, bf16)
    return x, gamma, beta, dy, add


@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("linear", [False, True], ids=["silu", "linear"])
def test_float64_formulas_are_group_norm_and_autograd(shape, linear):
    N, V, C, G = shape
    x, gamma, beta, dy, add = _case("mixed_offsets", shape, False)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.group_norm(xr.permute(0, 2, 1), G, gr, br, B.EPS).permute(0, 2, 1)
    y = y if linear else F.silu(y)
    y.backward(dy)
    fw = B.fwd(x, gamma, beta, G, D_CPU, linear, False)
    assert (fw.y - y.detach()).abs().max().item() <= 1e-12 * (1 + y.detach().abs().max().item())
    dyh, _ = B.dyh_stage(fw, dy, linear, False)
    bw = B.bwd(x, dyh, gamma, G, D_CPU, D_CPU, False, add=add)
    for got, ref in ((bw.dx, xr.grad + add), (bw.dgamma, gr.grad), (bw.dbeta, br.grad), (bw.colsum, (xr.grad + add).sum(1))):
        assert (got - ref).abs().max().item() <= 1e-10 * (1 + ref.abs().max().item())


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS, ids=[str(k) for k in KINDS])
def test_fp32_raw_moment_evaluation_stays_inside_every_bound(kind, bf16):
    worst = {}
    for i, shape in enumerate(SHAPES):
        N, V, C, G = shape
        x, gamma, beta, dy, add = _case(kind, shape, bf16, seed=i)
        for linear in (False, True):
            fw = B.fwd(x, gamma, beta, G, D_CPU, linear, bf16)
            y = B.f32_fwd(x, gamma, beta, G, linear, bf16).double()
            ref_dyh, b_dyh = B.dyh_stage(fw, dy, linear, bf16)
            dyh = B.f32_dyh(x, dy, gamma, beta, G, linear, bf16).double()
            bw = B.bwd(x, ref_dyh, gamma, G, D_CPU, D_CPU, bf16, dyh_err=b_dyh, add=add)
            dx, dgam, dbet, cs = B.f32_bwd(x, dyh, gamma, G, bf16, add=add)
            for name, got, ref, bound in (("y", y, fw.y, fw.bound), ("dyh", dyh, ref_dyh, b_dyh), ("dx", dx.double(), bw.dx, bw.b_dx),
                                          ("dgamma", dgam.double(), bw.dgamma, bw.b_dgamma), ("dbeta", dbet.double(), bw.dbeta, bw.b_dbeta),
                                          ("colsum", cs.double(), bw.colsum, bw.b_colsum)):
                err = (got - ref).abs()
                assert torch.isfinite(got).all() and torch.isfinite(bound).all(), (name, shape)
                ratio = (err / bound.clamp_min(1e-300)).max().item() if err.max().item() > 0 else 0.0
                worst[name] = max(worst.get(name, 0.0), ratio)
                assert (err <= bound).all(), f"{name} {shape} linear={linear}: err / bound {ratio:.3f}"
    print(f"cpu fp32 {kind} {'bf16' if bf16 else 'f32'}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_bound_rejects_a_reference_without_eps(bf16):
    """A group of std 0.01 around 0: rstd with eps is (1e-4 + 1e-5)^-1/2, without it 4.9 % larger.  The forward bound at |mean| / std = 0
    must not let that through (in bf16 storage too: 4.9 % is 12 times bf16's rounding error of 2^-8)."""
    N, V, C, G = 2, 240, 64, 8
    x, gamma, beta, _, _ = _case("tiny_std", (N, V, C, G), bf16)
    fw = B.fwd(x, gamma, beta, G, D_CPU, True, bf16)
    xr = x.reshape(N, V, G, C // G)
    no_eps = ((xr - fw.M.m[:, None, :, None]) / fw.M.v.sqrt()[:, None, :, None] * gamma.reshape(1, 1, G, -1) + beta.reshape(1, 1, G, -1)).reshape(N, V, C)
    bad = ((no_eps - fw.y).abs() > fw.bound).reshape(N, V, G, -1)
    assert bad[:, :, 0].float().mean().item() > 0.5, "the bound accepts a GroupNorm without eps on the std-0.01 group"


def test_chain_lengths_of_the_cpu_table():
    assert B.blocks_per_sample(32768 * 48, 48, 3) == 681 and B.blocks_per_sample(32768 * 48, 48, 3) * 3 <= 2048
    assert B.blocks_per_sample(105 * 24, 24, 1) == 3 and B.blocks_per_sample(4096 * 8, 8, 2) == 16
    assert B.fold_chain(7, 12) == 1 + 21 and B.fold_chain(1000, 8) == 32 + 3 + 4 and B.dot_sums_chain(4096) == 25


def test_gn_stats_refuses_wide_groups_from_partials(hip_lib):
    """More than 256 channels per group with conv partials: tile_partials_fold<256> has one thread per channel of a group.  Refused
    before any launch, the message names the limit."""
    f = hip_lib.vdm_gn_stats
    for c, groups, dtype in ((512, 1, 1), (512, 1, 0), (384, 1, 1)):            # (two sources cannot reach it: c1 + c2 <= 512)
        st = f(PTR, c, None, 0, 2, 64, groups, dtype, PTR, PTR, PTR, 5, None, 0, None, None)
        assert st == ERR_ARG, (c, groups)
        msg = hip_lib.vdm_last_error()
        assert b"channels per group" in msg and b"256" in msg, msg


def test_gn_stats_refuses_a_pass_that_outgrows_its_workspace(hip_lib):
    """n * workgroups-per-sample rows of 2 * groups floats must fit VDM_GN_STATS_WS_BYTES: with 48 pieces per voxel the per-sample count
    is a multiple of 3, so n = 2048 needs 6144 rows of 128 floats.  Refused before any launch; the message names the limit."""
    from vdm4cdm_amd import _lib
    f = hip_lib.vdm_gn_stats
    st = f(PTR, 192, None, 0, 2048, 8, 64, 0, PTR, PTR, None, 0, None, 0, None, None)
    assert st == ERR_ARG
    msg = hip_lib.vdm_last_error()
    assert b"VDM_GN_STATS_WS_BYTES" in msg and str(_lib.GN_STATS_WS_BYTES).encode() in msg, msg
    # second source over the limit, first one from partials
    st = f(None, 64, PTR, 192, 2048, 8, 64, 0, PTR, PTR, PTR, 3, None, 0, None, None)
    assert st == ERR_ARG and b"VDM_GN_STATS_WS_BYTES" in hip_lib.vdm_last_error()
