"""Learned-linear VDM training on the HIP backend and the network input gradients it rests on (K1t conv_in input gradient, K7b schedule
sums, K6i conditioning-MLP input gradients) against the CPU oracle (oracle/unet_oracle, oracle/vdm_oracle under torch autograd).

Tolerances as test_unet_gpu.py: fp32 storage - gradients <= 2e-3 * max|ref| + 1e-6 per tensor; bf16 storage - cosine similarity."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from helpers import grf, oracle_cfg, oracle_params, randomize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_net(D=16, chs=(16, 32, 64), sc=1, vd=(6,), pm="zeros", precision="fp32", seed=1):
    from vdm4cdm_amd.networks import CUNet
    net = CUNet(shape=(1, D, D, D), chs=list(chs), s_conditioning_channels=sc, v_conditioning_dims=list(vd), t_conditioning=True,
                norm_groups=8, mid_attn=False, dropout_prob=0.0, conv_padding_mode=pm, n_attention_heads=4, backend="hip",
                precision=precision)
    randomize(net, seed)
    return net


def inputs(net, B, seed=3):
    D = net.shape[1]
    x = grf((B, 1, D, D, D), seed)
    s = grf((B, 1, D, D, D), seed + 1) if net.s_conditioning_channels else None
    g = torch.Generator().manual_seed(seed + 2)
    t = torch.rand(B, generator=g)
    v = [torch.rand(B, d, generator=g) for d in net.v_conditioning_dims]
    return x, t, s, v


def _leaf(a, dev=None):
    return None if a is None else (a.to(dev) if dev else a.clone()).detach().requires_grad_(True)


def _close(got, ref, rel=2e-3):
    return (got - ref).abs().max().item() <= rel * ref.abs().max().item() + 1e-6


IN_CFGS = [dict(D=16, chs=(16, 32, 64), sc=1, vd=(6,), pm="zeros"),
           dict(D=16, chs=(48, 96), sc=1, vd=(6,), pm="circular"),
           dict(D=24, chs=(16, 32), sc=0, vd=(6, 3), pm="zeros")]


@pytest.mark.parametrize("cfg,precision", [(c, "fp32") for c in IN_CFGS] + [(IN_CFGS[0], "bf16")],
                         ids=["fp32_cfg0", "fp32_c48_circular", "fp32_nos_two_v", "bf16_cfg0"])
def test_input_gradients_match_oracle(cfg, precision):
    """d (sum w * eps_hat) / d {x, s_conditioning, t, v}: HIP backward (K1t + K6i) vs torch.autograd through the oracle."""
    from oracle import unet_oracle
    net = make_net(precision=precision, **cfg).to(DEV).train()
    x, t, s, v = inputs(net, 2)
    w = grf((2, 1) + net.shape[1:], 77) + 0.5
    xd, td, sd, vd = _leaf(x, DEV), _leaf(t, DEV), _leaf(s, DEV), [_leaf(a, DEV) for a in v]
    y = net(xd, t=td, s_conditioning=sd, v_conditionings=vd)
    (y * w.to(DEV)).sum().backward()
    xr, tr, sr, vr = _leaf(x), _leaf(t), _leaf(s), [_leaf(a) for a in v]
    yr = unet_oracle.cunet_forward(oracle_params(net), oracle_cfg(net), xr, tr, sr, vr)
    (yr * w).sum().backward()
    pairs = [("x", xd, xr), ("t", td, tr)] + ([("s", sd, sr)] if s is not None else []) + [(f"v{j}", a, b) for j, (a, b) in enumerate(zip(vd, vr))]
    for name, a, b in pairs:
        assert a.grad is not None, f"no gradient for {name}"
        got, ref = a.grad.cpu(), b.grad
        assert ref.abs().max().item() > 0, name
        if precision == "fp32":
            assert _close(got, ref), f"{name}: err {(got - ref).abs().max().item():.3e} vs max|ref| {ref.abs().max().item():.3e}"
        else:
            cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
            assert cos >= 0.99, f"{name}: cosine {cos}"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_parameter_gradients_unaffected_by_input_gradients(precision):
    """flat.grad with and without input gradients requested: bit-equal where the same kernels run (fp32: the fused tail is bf16-only),
    within the bf16 backward tolerance where the unfused tail replaces it."""
    net = make_net(precision=precision).to(DEV).train()
    x, t, s, v = inputs(net, 2)
    w = grf((2, 1) + net.shape[1:], 77).to(DEV) + 0.5
    grads = []
    for want in (False, True):
        net.zero_grad()
        xd = x.to(DEV).requires_grad_(want)
        y = net(xd, t=t.to(DEV).requires_grad_(want), s_conditioning=s.to(DEV), v_conditionings=[a.to(DEV) for a in v])
        (y * w).sum().backward()
        assert (xd.grad is not None) == want
        grads.append(net.flat.grad.detach().clone())
    if precision == "fp32":
        assert torch.equal(grads[0], grads[1])
    else:
        g0, g1 = oracle_params(net, flat=grads[0]), oracle_params(net, flat=grads[1])
        bad = [(k, c) for k, c in ((k, torch.nn.functional.cosine_similarity(g0[k].flatten(), g1[k].flatten(), dim=0).item())
                                   for k in g0 if g0[k].numel() >= 8) if c < 0.999]
        assert not bad, bad[:8]


def _learned_vdm(net, b, w):
    from vdm4cdm_amd.vdm_model import LightVDM
    vdm = LightVDM(score_model=net, draw_figure=None, gamma_min=-13.3, gamma_max=13.3, noise_schedule="learned_linear").to(DEV).train()
    with torch.no_grad():
        vdm.model.gamma_b.fill_(b)
        vdm.model.gamma_w.fill_(w)
    return vdm


def _learned_step(vdm, x, s, v, times=None, eps=None, eps0=None):
    vdm.zero_grad(set_to_none=True)
    loss, metrics = vdm.model.get_loss(x, times=times, eps=eps, eps0=eps0, s_conditioning=s, v_conditionings=v)
    loss.backward()
    m = vdm.model
    return (loss.detach().clone(), m.gamma_b.grad.detach().clone(), m.gamma_w.grad.detach().clone(),
            m.score_model.flat.grad.detach().clone(), metrics)


@pytest.mark.parametrize("w", [26.6 - 1.1, -(26.6 - 1.1)], ids=["w_pos", "w_neg"])
def test_learned_loss_and_gradients_match_oracle(w):
    """Supplied times / eps / eps0, fp32, D=16: the loss parts, dL/d gamma_b, dL/d gamma_w (the sign of |w| included) and every
    parameter gradient against vdm_oracle.vdm_loss with Schedule(kind="learned_linear") under fp64 autograd of b and w."""
    from oracle import unet_oracle, vdm_oracle
    b = -13.3 + 0.7
    net = make_net()
    vdm = _learned_vdm(net, b, w)
    x, _, s, v = inputs(net, 2)
    times = torch.tensor([0.3, 0.8])
    eps, eps0 = grf(x.shape, 50, slope=0.0), grf(x.shape, 51, slope=0.0)
    loss, gb, gw, gflat, metrics = _learned_step(vdm, x.to(DEV), s.to(DEV), [a.to(DEV) for a in v], times.to(DEV), eps.to(DEV), eps0.to(DEV))
    sched = vdm_oracle.Schedule(-13.3, 13.3, kind="learned_linear", b=b, w=w)
    sched.b.requires_grad_(True)
    sched.w.requires_grad_(True)
    P = {k: a.clone().requires_grad_(True) for k, a in oracle_params(net).items()}
    ref = vdm_oracle.vdm_loss(lambda z, tn: unet_oracle.cunet_forward(P, oracle_cfg(net), z, tn, s, v), sched, x, times.double(), eps, eps0)
    ref["elbo"].backward()
    for k in ("elbo", "diffusion_loss", "latent_loss", "reconstruction_loss"):
        assert metrics[k].item() == pytest.approx(ref[k].item(), rel=2e-4), k
    for name, got, r in (("gamma_b", gb, sched.b.grad), ("gamma_w", gw, sched.w.grad)):
        assert abs(got.item() - r.item()) <= 5e-3 * abs(r.item()) + 1e-5, f"{name}: {got.item()} vs oracle {r.item()}"
    assert math.copysign(1.0, gw.item()) == math.copysign(1.0, sched.w.grad.item())
    got = oracle_params(net, flat=gflat)
    bad = [(k, (got[k] - g.grad).abs().max().item()) for k, g in P.items() if g.grad is not None and not _close(got[k], g.grad)]
    assert not bad, bad[:8]


def _fused_vs_supplied(vdm, x, s, v, times):
    from vdm4cdm_amd import hip_ops as ops
    from vdm4cdm_amd.vdm_model import noise_seed, reset_train_generators
    reset_train_generators()
    fused = _learned_step(vdm, x, s, v, times)                                   # eps / eps0 drawn inside the kernels
    reset_train_generators()
    eps = ops.randn(torch.empty_like(x), noise_seed(), 1)                       # the same fields, materialised (rank 0: streams 1, 2)
    eps0 = ops.randn(torch.empty_like(x), noise_seed(), 2)
    supplied = _learned_step(vdm, x, s, v, times, eps, eps0)
    return fused, supplied


def test_fused_head_equals_supplied_noise_and_is_reproducible():
    """eps=None (Philox in K7 / K8 / K7b) gives bit for bit the gradients of eps = ops.randn(same seed, stream); two identical learned
    steps give bit-identical gamma_b / gamma_w gradients."""
    net = make_net()
    vdm = _learned_vdm(net, -12.0, 25.0)
    x, _, s, v = inputs(net, 2)
    x, s, v = x.to(DEV), s.to(DEV), [a.to(DEV) for a in v]
    times = torch.tensor([0.2, 0.7], device=DEV)
    fused, supplied = _fused_vs_supplied(vdm, x, s, v, times)
    for a, b_ in zip(fused[:4], supplied[:4]):
        assert torch.equal(a, b_)
    again, _ = _fused_vs_supplied(vdm, x, s, v, times)
    assert torch.equal(fused[1], again[1]) and torch.equal(fused[2], again[2]) and torch.equal(fused[3], again[3])
    assert fused[1].item() != 0.0 and fused[2].item() != 0.0


def test_full_size_learned_step_bf16_vs_fp32_storage():
    """128^3, batch 2, chs (48, 96, 192, 384) - the train3D configuration: finite loss and gradients, b / w gradients of bf16 storage
    within 2 % of the fp32-storage run on the same weights, times and noise."""
    from vdm4cdm_amd import hip_ops as ops
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    D = 128
    bt = SyntheticAstroDataModule(cropsize=D, batch_size=2, seed=1000)._make_batch(1000, 2)
    x, s, v = bt["x"].to(DEV), bt["conditioning"].to(DEV), [bt["conditioning_values"][0].to(DEV)]
    eps, eps0 = ops.randn(torch.empty_like(x), 7, 1), ops.randn(torch.empty_like(x), 8, 2)
    times = torch.tensor([0.35, 0.85], device=DEV)
    out = {}
    for precision in ("bf16", "fp32"):
        net = make_net(D=D, chs=(48, 96, 192, 384), precision=precision, seed=4)
        vdm = _learned_vdm(net, -13.3, 26.6)
        loss, gb, gw, gflat, _ = _learned_step(vdm, x, s, v, times, eps, eps0)
        assert torch.isfinite(loss) and torch.isfinite(gb) and torch.isfinite(gw) and torch.isfinite(gflat).all()
        out[precision] = (gb.item(), gw.item())
        del vdm, net, gflat
        torch.cuda.empty_cache()
    for i, name in enumerate(("gamma_b", "gamma_w")):
        a, r = out["bf16"][i], out["fp32"][i]
        assert abs(a - r) <= 0.02 * abs(r), f"{name}: bf16 {a} vs fp32 {r}"


def test_learned_training_with_trainer_and_state_dict_roundtrip(tmp_path):
    """~20 Trainer steps of learned-linear on HIP (32^3): the loss goes down and gamma_b / gamma_w move; state_dict -> load_state_dict
    into a fresh model -> draw_samples with the same seed gives the same cube."""
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    from vdm4cdm_amd.trainer import Trainer
    from vdm4cdm_amd.vdm_model import LightVDM
    torch.manual_seed(0)
    net = make_net(D=32, seed=21)
    vdm = LightVDM(score_model=net, draw_figure=None, gamma_min=-13.3, gamma_max=13.3, noise_schedule="learned_linear", learning_rate=3e-3)
    b0, w0 = vdm.model.gamma_b.item(), vdm.model.gamma_w.item()
    dm = SyntheticAstroDataModule(cropsize=32, batch_size=2, n_train=2, seed=5)
    tr = Trainer(max_steps=20, val_check_interval=0, gradient_clip_val=0.5, every_n_train_steps=0, default_root_dir=str(tmp_path),
                 experiment_name="learned", device="cuda", enable_progress=False, log_every_n_steps=1)
    tr.fit(vdm, dm)
    losses = [json.loads(l)["loss"] for l in open(tmp_path / "learned" / "metrics.jsonl") if '"loss"' in l]
    assert len(losses) >= 15 and all(math.isfinite(l) for l in losses)
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5, losses
    assert vdm.model.gamma_b.item() != b0 and vdm.model.gamma_w.item() != w0
    sd = vdm.state_dict()
    assert "model.gamma_b" in sd and "model.gamma_w" in sd
    net2 = make_net(D=32, seed=99)
    vdm2 = LightVDM(score_model=net2, draw_figure=None, gamma_min=-13.3, gamma_max=13.3, noise_schedule="learned_linear").to(DEV)
    vdm2.load_state_dict(sd)
    vdm.eval()
    vdm2.eval()
    bt = dm._make_batch(7, 1)
    kw = dict(s_conditioning=bt["conditioning"].to(DEV), v_conditionings=[bt["conditioning_values"][0].to(DEV)])
    a = vdm.draw_samples(batch_size=1, n_sampling_steps=4, seed=123, **kw)
    b = vdm2.draw_samples(batch_size=1, n_sampling_steps=4, seed=123, **kw)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_train3d_entry_point_runs(tmp_path):
    env = dict(os.environ, VDM4CDM_MAX_STEPS="3", VDM4CDM_LOG_DIR=str(tmp_path), VDM4CDM_PRECISION="bf16")
    env.pop("VDM4CDM_DATA_ROOT", None)                   # the synthetic data fallback
    r = subprocess.run(["timeout", "-k", "10", "500", sys.executable, os.path.join(ROOT, "train3D_c_c_from_field_name.py"), "Mstar", "Mcdm"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, r.stderr[-2000:]
    log = tmp_path / "LH_c_uc_Mstar_to_Mcdm" / "metrics.jsonl"
    assert log.exists() and "train/elbo" in log.read_text()
