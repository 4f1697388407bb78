"""Shared by test_ddnm_graph_cpu.py / test_ddnm_graph_gpu.py: the DDNM fixture cases (tests/golden/make_ddnm_golden.py) set up for
get_ddnm_result's noises= / operator= keywords."""
import torch

from helpers import DD, DDNM_GOLD


def fixture_noises(case):
    """The fixture's noise stream as a list, z_1 first: every draw of the reference loop has the cube batch's shape, the count is the
    fixture's noise_calls."""
    name, D, chs, seed, B, n, l, op, cond = case
    g = torch.Generator().manual_seed(DD.NOISE_SEED + seed)
    return [torch.randn((B, 1, D, D, D), generator=g) for _ in range(int(DDNM_GOLD[f"{name}/noise_calls"][0]))]


def fixture_vdm(case, device, backend, precision="fp32", w_cfg=None):
    """(vdm, y, kwargs) of a fixture case on `device`: the product CUNet with the fixture's seeded weights."""
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.vdm_model import LightVDM
    net0, y, kwargs = DD.case_inputs(case, DDNM_GOLD)
    net = CUNet(shape=net0.shape, chs=net0.chs, s_conditioning_channels=net0.s_conditioning_channels,
                v_conditioning_dims=net0.v_conditioning_dims, norm_groups=8, backend=backend, precision=precision)
    with torch.no_grad():
        net.flat.copy_(net0.flat)
    vdm = LightVDM(score_model=net, gamma_max=13.3, w_cfg=w_cfg).to(device).eval()
    kw = {k: ([a.to(device) for a in v] if isinstance(v, list) else v.to(device)) for k, v in kwargs.items()}
    return vdm, y.to(device), kw


def fixture_operator(case, device):
    """The built-in operator that matches the fixture's callables: mask = the half-cube mask, pool = 2x block mean along x."""
    from vdm4cdm_amd import utils
    name, D, chs, seed, B, n, l, op, cond = case
    if op == "mask":
        m = torch.zeros((B, 1, D, D, D))
        m[..., : D // 2] = 1.0
        return utils.MaskOperator(m)
    return utils.BlockMeanOperator((1, 1, 2))


def residual(A, x, y):
    """Range-space consistency max|A x - y| / max(1, max|y|), as helpers.replay_ddnm_case."""
    return (A(x) - y).abs().max().item() / max(1.0, y.abs().max().item())
