"""GPU tests of the HIP CUNet conditioned on K = 2, 3 fields at once (s_conditioning [B, K, D, H, W]): forward, backward and input
gradients against the CPU oracle, VDM.get_loss (fused head, unfused head, learned schedule, graph-captured step) and the samplers
(ancestral, classifier-free guidance, batched seeds, DDNM) on the captured-graph path.

Tolerances are those stated at the top of tests/test_unet_gpu.py: fp32 forward 2e-4 max|ref|, fp32 gradients 2e-3 max|ref grad| + 1e-6 per
tensor, bf16 forward 3e-2 max|ref| with cosine > 0.9995, bf16 gradients cosine >= 0.995; loss parts rel 2e-4; sampler 2e-5 max|ref| + 1e-3.
K = 1 through the public interface calls the entries it called before (tests/test_unet_gpu.py and the other existing files guard it).
"""
import pytest
import torch

from helpers import grf, oracle_cfg, oracle_params, randomize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 16
cosine = lambda a, b: torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()


def make_net(K, chs=(16, 32), pm="zeros", precision="fp32", vd=(6,), dropout=0.0, seed=1, backend="hip", zero_init_std=0.05, d=D):
    from vdm4cdm_amd.networks import CUNet
    net = CUNet(shape=(1, d, d, d), chs=list(chs), s_conditioning_channels=K, v_conditioning_dims=list(vd), t_conditioning=True,
                norm_groups=8, mid_attn=False, dropout_prob=dropout, conv_padding_mode=pm, n_attention_heads=4, backend=backend,
                precision=precision)
    return randomize(net, seed, zero_init_std=zero_init_std)


def make_vdm(net, **kw):
    from vdm4cdm_amd.vdm_model import LightVDM
    return LightVDM(score_model=net, draw_figure=None, gamma_max=13.3, learning_rate=3e-4, **kw)


def inputs(net, B, seed=3):
    K, d = net.s_conditioning_channels, net.shape[1]
    x = grf((B, 1, d, d, d), seed)
    s = torch.cat([grf((B, 1, d, d, d), seed + 10 + j) for j in range(K)], dim=1)          # K distinct fields
    g = torch.Generator().manual_seed(seed + 2)
    t = torch.rand(B, generator=g)
    v = [torch.rand(B, n, generator=g) for n in net.v_conditioning_dims]
    return x, t, s, v


def oracle_forward(net, x, t, s, v, params=None):
    from oracle import unet_oracle
    return unet_oracle.cunet_forward(oracle_params(net) if params is None else params, oracle_cfg(net), x, t, s, v)


def hip_forward(net, x, t, s, v):
    return net(x.to(DEV), t=t.to(DEV), s_conditioning=s.to(DEV), v_conditionings=[a.to(DEV) for a in v])


_REF = {}


def reference(K, chs, pm):
    """Oracle forward and autograd of one configuration, computed once and shared by the fp32 and bf16 cases (never modified)."""
    key = (K, chs, pm)
    if key not in _REF:
        net = make_net(K, chs, pm)
        x, t, s, v = inputs(net, 2)
        w = grf((2, 1, D, D, D), 77) + 0.5
        p = {k: a.clone().requires_grad_(True) for k, a in oracle_params(net).items()}
        xr, sr = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
        y = oracle_forward(net, xr, t, sr, v, params=p)
        (y * w).sum().backward()
        _REF[key] = (y.detach(), {k: a.grad for k, a in p.items()}, xr.grad, sr.grad, w)
    return _REF[key]


CASES = [(K, chs, pm) for K in (2, 3) for chs in ((16, 32), (16, 32, 64)) for pm in ("zeros", "circular")]
CASE_IDS = [f"K{k}_{'x'.join(map(str, c))}_{p}" for k, c, p in CASES]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("K,chs,pm", CASES, ids=CASE_IDS)
def test_forward_backward_and_input_gradients_match_oracle(K, chs, pm, precision):
    """Forward, every parameter gradient (conv_in.weight per input channel: a swapped or dropped channel cannot hide in the tensor
    maximum), dz and all K planes of ds against oracle autograd."""
    yr, gref, dxr, dsr, w = reference(K, chs, pm)
    net = make_net(K, chs, pm, precision).to(DEV).train()
    x, t, s, v = inputs(net, 2)
    xd, sd = x.to(DEV).requires_grad_(True), s.to(DEV).requires_grad_(True)
    y = net(xd, t=t.to(DEV), s_conditioning=sd, v_conditionings=[a.to(DEV) for a in v])
    (y * w.to(DEV)).sum().backward()
    y, got = y.detach().cpu(), oracle_params(net, flat=net.flat.grad.detach().cpu())
    assert sd.grad is not None and sd.grad.shape == (2, K, D, D, D) and xd.grad.shape == x.shape
    assert gref["conv_in.weight"].shape[1] == 1 + K
    pairs = [(k, got[k], g) for k, g in gref.items() if g is not None and k != "conv_in.weight"]
    pairs += [(f"conv_in.weight[:, {c}]", got["conv_in.weight"][:, c], gref["conv_in.weight"][:, c]) for c in range(1 + K)]
    ins = [("dz", xd.grad.cpu(), dxr)] + [(f"ds[:, {j}]", sd.grad[:, j].cpu(), dsr[:, j]) for j in range(K)]
    ferr = (y - yr).abs().max().item()
    if precision == "fp32":
        assert ferr <= 2e-4 * yr.abs().max().item(), f"forward err {ferr} vs max {yr.abs().max().item()}"
        bad = [(k, (a - g).abs().max().item(), g.abs().max().item()) for k, a, g in pairs + ins
               if (a - g).abs().max().item() > 2e-3 * max(g.abs().max().item(), 1e-8) + 1e-6]
    else:
        assert ferr <= 3e-2 * yr.abs().max().item() and cosine(y, yr) > 0.9995, (ferr, cosine(y, yr))
        bad = [(k, cosine(a, g)) for k, a, g in pairs + ins if g.numel() >= 8 and cosine(a, g) < 0.995]
    assert all(g.abs().max().item() > 0 for _, _, g in ins), "a reference input gradient is zero: the check would be vacuous"
    assert not bad, f"{len(bad)} tensors off: {bad[:8]}"


def test_no_conditioning_gradient_without_requires_grad(monkeypatch):
    """z.requires_grad alone: n_ds = 0 reaches the entry (dz only) and dz has the bits of the call that also asks for ds."""
    from vdm4cdm_amd import hip_ops as ops
    net = make_net(2).to(DEV).train()
    x, t, s, v = inputs(net, 2)
    seen, real = [], ops.conv_in_dgrad_fields

    def spy(dh, weight, cin, circular, want_s):
        seen.append((cin, want_s))
        return real(dh, weight, cin, circular, want_s)
    monkeypatch.setattr(ops, "conv_in_dgrad_fields", spy)
    grads = []
    for want in (False, True):
        xd, sd = x.to(DEV).requires_grad_(True), s.to(DEV).requires_grad_(want)
        net.zero_grad()
        net(xd, t=t.to(DEV), s_conditioning=sd, v_conditionings=[a.to(DEV) for a in v]).sum().backward()
        assert (sd.grad is not None) == want
        grads.append(xd.grad.clone())
    assert seen == [(3, False), (3, True)] and torch.equal(grads[0], grads[1])


def test_unsupported_configurations_still_raise():
    from vdm4cdm_amd.networks import CUNet
    x = torch.zeros(1, 1, D, D, D, device=DEV)
    net4 = make_net(4).to(DEV).eval()
    with pytest.raises(NotImplementedError, match="s_conditioning_channels<=3"):
        net4(x, t=torch.zeros(1, device=DEV), s_conditioning=torch.zeros(1, 4, D, D, D, device=DEV), v_conditionings=[torch.zeros(1, 6, device=DEV)])
    net2 = CUNet(shape=(2, D, D, D), chs=[16, 32], s_conditioning_channels=1, v_conditioning_dims=[], norm_groups=8, backend="hip",
                 precision="fp32").to(DEV).eval()
    with pytest.raises(NotImplementedError):
        net2(torch.zeros(1, 2, D, D, D, device=DEV), t=torch.zeros(1, device=DEV), s_conditioning=torch.zeros(1, 1, D, D, D, device=DEV))


# ------------------------------------------------------------------------------------------ VDM.get_loss
def _reseed(seed=9):
    import vdm4cdm_amd.unet_hip as uh
    import vdm4cdm_amd.vdm_model as vm
    torch.manual_seed(seed)
    uh._seed_counter[0] = 0
    vm.reset_train_generators()


@pytest.mark.parametrize("K", [2, 3])
def test_fused_head_equals_unfused_head_fp32(K, monkeypatch):
    """The fused head (vdm_diffuse_pack_fields) and VDM4CDM_EXPERIMENT=fused_head=0 (randn -> diffuse -> vdm_pack_fields) from the same generator
    state: the same loss, ELBO parts and parameter gradient, bit for bit."""
    import vdm4cdm_amd.vdm_model as vm
    net = make_net(K, dropout=0.1)
    vdm = make_vdm(net).to(DEV).train()
    x, _, s, v = inputs(net, 2)
    kw = dict(s_conditioning=s.to(DEV), v_conditionings=[a.to(DEV) for a in v])
    res = []
    for fused in (True, False):
        monkeypatch.setattr(vm, "FUSED_HEAD", fused)
        _reseed()
        net.flat.grad = None
        loss, metrics = vdm.model.get_loss(x.to(DEV), **kw)
        loss.backward()
        res.append((loss.detach().clone(), {k: m.clone() for k, m in metrics.items()}, net.flat.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])
    assert torch.equal(res[0][2], res[1][2]) and torch.isfinite(res[0][2]).all() and res[0][2].abs().max().item() > 0


def test_loss_matches_oracle_for_supplied_noise():
    from oracle import unet_oracle, vdm_oracle
    net = make_net(3, chs=(16, 32, 64))
    vdm = make_vdm(net).to(DEV).train()
    x, _, s, v = inputs(net, 2)
    times = torch.tensor([0.3, 0.8])
    eps, eps0 = grf(x.shape, 50, slope=0.0), grf(x.shape, 51, slope=0.0)
    loss, metrics = vdm.model.get_loss(x.to(DEV), times=times.to(DEV), eps=eps.to(DEV), eps0=eps0.to(DEV), s_conditioning=s.to(DEV),
                                       v_conditionings=[a.to(DEV) for a in v])
    P = oracle_params(net)
    score = lambda z, tn: unet_oracle.cunet_forward(P, oracle_cfg(net), z, tn, s, v)
    ref = vdm_oracle.vdm_loss(score, vdm_oracle.Schedule(-13.3, 13.3), x, times.double(), eps, eps0)
    for k in ("elbo", "diffusion_loss", "latent_loss", "reconstruction_loss"):
        assert metrics[k].item() == pytest.approx(ref[k].item(), rel=2e-4), k
    loss.backward()
    assert torch.isfinite(net.flat.grad).all() and net.flat.grad.abs().max().item() > 0


def test_learned_linear_schedule_matches_the_torch_backend():
    """noise_schedule="learned_linear" with K = 2 (fused head through _LearnedDiffuseFn, K1t dz through vdm_conv_in_dgrad_fields): finite
    gradients of gamma_b / gamma_w that agree with the torch backend (same weights, supplied times / eps / eps0) at the fp32 gradient
    tolerance; with the noise drawn in the kernels the step runs too."""
    b, w = -13.3 + 0.7, 26.6 - 1.1
    x, _, s, v = inputs(make_net(2), 2)
    times = torch.tensor([0.3, 0.8])
    eps, eps0 = grf(x.shape, 50, slope=0.0), grf(x.shape, 51, slope=0.0)
    out = {}
    for backend, dev in (("torch", "cpu"), ("hip", DEV)):
        vdm = make_vdm(make_net(2, backend=backend), gamma_min=-13.3, noise_schedule="learned_linear").to(dev).train()
        with torch.no_grad():
            vdm.model.gamma_b.fill_(b)
            vdm.model.gamma_w.fill_(w)
        loss, _ = vdm.model.get_loss(x.to(dev), times=times.to(dev), eps=eps.to(dev), eps0=eps0.to(dev), s_conditioning=s.to(dev),
                                     v_conditionings=[a.to(dev) for a in v])
        loss.backward()
        out[backend] = (loss.item(), vdm.model.gamma_b.grad.item(), vdm.model.gamma_w.grad.item())
        if backend == "hip":
            vdm.zero_grad(set_to_none=True)
            loss2, _ = vdm.model.get_loss(x.to(dev), s_conditioning=s.to(dev), v_conditionings=[a.to(dev) for a in v])
            loss2.backward()
            assert all(torch.isfinite(g).all() for g in (loss2, vdm.model.gamma_b.grad, vdm.model.gamma_w.grad, vdm.model.score_model.flat.grad))
            assert vdm.model.gamma_b.grad.item() != 0.0 and vdm.model.gamma_w.grad.item() != 0.0
    assert out["hip"][0] == pytest.approx(out["torch"][0], rel=2e-4)
    for j, name in ((1, "gamma_b"), (2, "gamma_w")):          # one-element tensors: each against its own reference
        got, ref = out["hip"][j], out["torch"][j]
        print(f"{name}: hip {got!r} torch backend {ref!r} rel err {abs(got - ref) / abs(ref):.3e}")
        assert ref != 0.0 and abs(got - ref) <= 2e-3 * abs(ref) + 1e-6, f"{name}: {got} vs torch backend {ref}"


def test_graph_captured_step_equals_the_eager_step():
    """K = 2, bf16, dropout on: the captured forward + backward, replayed, gives the loss and every parameter gradient of the eager
    step with the same host seeds and device step counter, bit for bit - at two values of the counter (two replays, two eager steps)."""
    import vdm4cdm_amd.vdm_model as vm
    from vdm4cdm_amd import hip_ops as ops
    try:
        net = make_net(2, chs=(16, 32, 64), precision="bf16", dropout=0.1, seed=8)
        vdm = make_vdm(net).to(DEV).train()
        x, t, s, v = inputs(net, 2, seed=5)
        batch = {"x": x.to(DEV), "conditioning": s.to(DEV), "conditioning_values": [a.to(DEV) for a in v]}
        counter = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.SEED_STEP = counter

        def fb():
            loss = vdm.training_step(batch, 0)
            net.flat.grad = None
            loss.backward()
            return loss

        def reseed(step):
            _reseed(5)
            vdm.model._graph_seed = 1234
            counter.fill_(step)

        eager = []
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fb()
            for step in (7, 8):
                reseed(step)
                le = fb()
                eager.append((le.detach().clone(), net.flat.grad.clone()))
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        reseed(7)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            lg = fb()
        for step, (le, ge) in zip((7, 8), eager):
            counter.fill_(step)
            g.replay()
            torch.cuda.synchronize()
            assert torch.isfinite(ge).all() and torch.equal(le, lg), (step, le.item(), lg.item())
            diff = [n for n in net.spec.items if not torch.equal(net.view(n, ge), net.view(n, net.flat.grad))]
            assert not diff, f"step {step}: captured step differs from the eager step in {len(diff)} gradient tensors: {diff[:8]}"
        assert not torch.equal(eager[0][0], eager[1][0])
        del g
    finally:
        ops.SEED_STEP = None


def test_graphed_train_step_with_two_fields():
    """trainer.GraphedTrainStep itself with K = 2 (the static copy of the [B, 2, ...] conditioning, warm-up and restore, clip + capturable
    AdamW and the re-packing of conv_in's cin = 3 weights inside the graph, the device counter), with what tests/test_resume_gpu.py and
    tests/test_unet_gpu.py assert of it: a used optimizer state, the parameters and the counter are put back after construction; two
    replays are optimizer steps 2 and 3 with counter == 2 and finite, different losses; the replay reads the batch it is given; eager
    steps afterwards do not see the counter; the packed weights follow the in-graph steps (forward against the oracle on the new weights)."""
    from vdm4cdm_amd import hip_ops as ops
    from vdm4cdm_amd.trainer import GraphedTrainStep, clip_grad_norm_flat_
    try:
        _reseed(11)
        net = make_net(2, dropout=0.1, seed=21)
        vdm = make_vdm(net).to(DEV).train()
        vdm.learning_rate = 3e-3
        params = [p for p in vdm.parameters() if p.requires_grad]
        opt = vdm.configure_optimizers(capturable=True)
        x, t, s, v = inputs(net, 2, seed=5)
        x2, _, s2, v2 = inputs(net, 2, seed=40)
        batch = {"x": x.to(DEV), "conditioning": s.to(DEV), "conditioning_values": [a.to(DEV) for a in v]}
        batch2 = {"x": x2.to(DEV), "conditioning": s2.to(DEV), "conditioning_values": [a.to(DEV) for a in v2]}
        loss = vdm.training_step(batch, 0)                      # one eager step: the optimizer state is not empty
        opt.zero_grad(set_to_none=True)
        loss.backward()
        clip_grad_norm_flat_(params, 0.5, True, want_norm=False)
        opt.step()
        del loss
        st = opt.state[net.flat]
        before = {k: a.detach().clone() for k, a in st.items()}
        flat = net.flat.detach().clone()
        assert float(before["step"]) == 1 and before["exp_avg"].abs().max().item() > 0
        gs = GraphedTrainStep(vdm, opt, params, 0.5, batch)
        assert sorted(st) == sorted(before) and all(torch.equal(st[k], before[k]) for k in before), "optimizer state not put back"
        assert torch.equal(net.flat.detach(), flat) and gs.counter.item() == 0 and ops.SEED_STEP is None
        assert gs.static["conditioning"].shape == (2, 2, D, D, D)
        l1 = gs(batch).detach().clone()
        flat1 = net.flat.detach().clone()
        l2 = gs(batch2).detach().clone()
        torch.cuda.synchronize()
        assert torch.equal(gs.static["conditioning"], batch2["conditioning"]) and torch.equal(gs.static["x"], batch2["x"])
        assert gs.counter.item() == 2 and gs.state_dict()["counter"] == 2 and gs.replays == 2 and float(st["step"]) == 3
        assert torch.isfinite(l1) and torch.isfinite(l2) and not torch.equal(l1, l2) and torch.isfinite(gs.gnorm).all()
        assert torch.isfinite(net.flat).all() and not torch.equal(flat1, flat) and not torch.equal(net.flat.detach(), flat1)
        assert not torch.equal(net.view("conv_in.weight").detach()[..., 2], net.view("conv_in.weight", flat)[..., 2]), "field 1 is not trained"
        assert ops.SEED_STEP is None
        e1, e2 = vdm.training_step(batch, 0).detach().clone(), vdm.training_step(batch, 0).detach().clone()
        assert not torch.equal(e1, e2) and gs.counter.item() == 2
        vdm.eval()
        with torch.no_grad():
            out = hip_forward(net, x, t, s, v).cpu()
        ref = oracle_forward(net, x, t, s, v)
        assert (out - ref).abs().max().item() <= 2e-4 * ref.abs().max().item(), "the packed weights do not follow the in-graph steps"
    finally:
        ops.SEED_STEP = None


# ------------------------------------------------------------------------------------------ sampling
def test_sampler_graph_equals_eager_and_batched_chains():
    """draw_samples, K = 2, 6 steps, seeds [1, 2]: the graph path and use_graph=False agree bit for bit; on a zero-output network (the
    condition tests/test_batched_sampling_gpu.py states for bit equality: the conv plans may differ with the batch size) chain 1 alone
    equals chain 1 in the batch, and on the random network to 1e-4 max|single| (fp32, that file's rounding bound)."""
    net = make_net(2)
    vdm = make_vdm(net).to(DEV).eval()
    _, _, s, v = inputs(net, 2)
    kw = dict(s_conditioning=s.to(DEV), v_conditionings=[a.to(DEV) for a in v])
    a = vdm.draw_samples(batch_size=2, n_sampling_steps=6, seeds=[1, 2], use_graph=True, **kw)
    b = vdm.draw_samples(batch_size=2, n_sampling_steps=6, seeds=[1, 2], use_graph=False, **kw)
    assert a.shape == (2, 1, D, D, D) and torch.isfinite(a).all() and torch.equal(a, b)
    kw1 = dict(s_conditioning=s[1:].to(DEV), v_conditionings=[c[1:].to(DEV) for c in v])
    one = vdm.draw_samples(batch_size=1, n_sampling_steps=6, seed=2, **kw1)
    assert (a[1:] - one).abs().max().item() <= 1e-4 * one.abs().max().item()
    with torch.no_grad():
        net.view("conv_out.weight").zero_()
        net.view("conv_out.bias").zero_()
    net.mark_weights_dirty()
    a0 = vdm.draw_samples(batch_size=2, n_sampling_steps=6, seeds=[1, 2], **kw)
    one0 = vdm.draw_samples(batch_size=1, n_sampling_steps=6, seed=2, **kw1)
    assert torch.equal(a0[1:], one0)


def test_sampler_matches_the_torch_backend_loop():
    """Supplied z_1 and noises: the HIP graph path against the torch backend's loop on the CPU (same weights), at the sampler tolerance
    of tests/test_unet_gpu.py; one conditioning cube [1, K, ...] serves both rows."""
    n, B = 6, 2
    net = make_net(2)
    ref_net = make_net(2, backend="torch")
    assert torch.equal(net.flat, ref_net.flat)
    x, _, s, v = inputs(net, 1)
    z1 = grf((B,) + tuple(x.shape[1:]), 60, slope=0.0)
    noises = [grf(z1.shape, 100 + i, slope=0.0) for i in range(n)]
    out = make_vdm(net).to(DEV).eval().draw_samples(batch_size=B, n_sampling_steps=n, z=z1.clone().to(DEV), noises=[a.to(DEV) for a in noises],
                                                     s_conditioning=s.to(DEV), v_conditionings=[a.to(DEV) for a in v]).cpu()
    ref = make_vdm(ref_net).eval().draw_samples(batch_size=B, n_sampling_steps=n, z=z1.clone(), noises=noises, s_conditioning=s,
                                                v_conditionings=v)
    err = (out - ref).abs().max().item()
    assert err <= 2e-5 * ref.abs().max().item() + 1e-3, f"sampler err {err} (max|ref| {ref.abs().max().item()})"


def test_classifier_free_guidance_is_the_blend_of_two_forwards():
    """w_cfg = 0.5: get_pred_noise (one batch-doubled forward with [2B, K, ...] conditioning) equals (1 + w) eps(v) - w eps(masked v) of
    two separate forwards; the guided sampler runs on the graph path and equals use_graph=False."""
    w = 0.5
    net = make_net(2)
    vdm = make_vdm(net, w_cfg=w).to(DEV).eval()
    x, _, s, v = inputs(net, 2)
    xd, sd, vd = x.to(DEV), s.to(DEV), [a.to(DEV) for a in v]
    with torch.no_grad():
        g_t = vdm.model.gamma(torch.tensor(0.6, device=DEV))
        e = vdm.model.get_pred_noise(xd, g_t, s_conditioning=sd, v_conditionings=vd)
        tn = ((g_t + 13.3) / 26.6).expand(2)
        e_c = net(xd, t=tn, s_conditioning=sd, v_conditionings=vd)
        e_u = net(xd, t=tn, s_conditioning=sd, v_conditionings=vdm.model.cfg_mask(vd))
    blend = (1.0 + w) * e_c - w * e_u
    assert (e_c - e_u).abs().max().item() > 1e-3 * e_c.abs().max().item(), "guidance has no effect: the check would be vacuous"
    assert (e - blend).abs().max().item() <= 1e-4 * blend.abs().max().item() + 1e-5          # (the conv plans differ with the batch size)
    a = vdm.draw_samples(batch_size=2, n_sampling_steps=6, seeds=[1, 2], use_graph=True, s_conditioning=sd, v_conditionings=vd)
    b = vdm.draw_samples(batch_size=2, n_sampling_steps=6, seeds=[1, 2], use_graph=False, s_conditioning=sd, v_conditionings=vd)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_ddnm_mask_graph_equals_eager():
    """One DDNM inpainting case with K = 2 (MaskOperator, seeds=[3], 6 steps): the graph path equals use_graph=False bit for bit."""
    from vdm4cdm_amd import utils
    net = make_net(2)
    vdm = make_vdm(net).to(DEV).eval()
    x, _, s, v = inputs(net, 1)
    mask = torch.zeros(1, 1, D, D, D)
    mask[..., : D // 2, :] = 1.0
    op = utils.MaskOperator(mask)
    y = op.A(x).to(DEV)
    kw = dict(operator=op, n_sampling_steps=6, l=2, seeds=[3], s_conditioning=s.to(DEV), v_conditionings=[a.to(DEV) for a in v])
    stats = {}
    a = utils.get_ddnm_result(vdm, y, use_graph=True, stats=stats, **kw)
    b = utils.get_ddnm_result(vdm, y, use_graph=False, **kw)
    assert stats.get("graph") and a.shape == x.shape and torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------------------------------ data path
def test_file_backed_module_batches_three_fields_in_one_launch(tmp_path, monkeypatch):
    """Mstar + Mgas -> Mcdm from stacks on disk (Mgas' constants from $VDM4CDM_NORMALIZATIONS): one vdm_augment_batch launch per batch for
    all three channels; with the same seed (the same crops, flips and permutations) conditioning[:, j] and x have the bits of the
    single-field modules' batches."""
    import json
    import numpy as np
    from vdm4cdm_amd import data, hip_ops
    root = data.write_synthetic_camels(str(tmp_path / "root"), dataset_name="CMD_128", n_sims=3, fullsize=16, seed=1)
    star = np.load(data.field_path(root, "CMD_128", "Astrid", "LH", "z_0.0", "Mstar"))
    np.save(data.field_path(root, "CMD_128", "Astrid", "LH", "z_0.0", "Mgas"), (3.0 * star[:, ::-1] + 1.0).astype(np.float32))
    (tmp_path / "norm.json").write_text(json.dumps({"Mgas_m": 0.4, "Mgas_s": 0.25}))
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, str(tmp_path / "norm.json"))
    launches, real = [], hip_ops.augment_batch

    def counted(fields, *a, **k):
        launches.append(len(fields))
        return real(fields, *a, **k)
    monkeypatch.setattr(hip_ops, "augment_batch", counted)

    def first_batch(names):
        dm = data.get_dataset(dataset_name="CMD_128", return_func=data.cond_return_func(len(names) - 1), set_name="LH", channel_names=names,
                              stage="fit", batch_size=2, cropsize=8, data_root=root, seed=1)
        dm.device = DEV
        return next(iter(dm.train_dataloader()))
    b3 = first_batch(["Mstar", "Mgas", "Mcdm"])
    assert launches == [3] and b3["conditioning"].shape == (2, 2, 8, 8, 8) and b3["x"].shape == (2, 1, 8, 8, 8) and b3["x"].is_cuda
    for j, name in enumerate(["Mstar", "Mgas"]):
        b2 = first_batch([name, "Mcdm"])
        assert torch.equal(b2["conditioning"], b3["conditioning"][:, j:j + 1]), name
        assert torch.equal(b2["x"], b3["x"]) and torch.equal(b2["conditioning_values"][0], b3["conditioning_values"][0])
    assert not torch.equal(b3["conditioning"][:, 0], b3["conditioning"][:, 1])


def test_derived_module_with_four_names_equals_the_single_field_modules(tmp_path, monkeypatch):
    """$VDM4CDM_DOWNGRID=1 with four channel names (Mstar + Mgas + T -> Mcdm): only the 256-named stacks exist, every field is down-gridded
    in HBM (16 -> 8 here), one augment launch serves the four channels, and conditioning[:, j] / x have the bits of the two-name derived
    modules with the same seed."""
    import json
    import numpy as np
    from vdm4cdm_amd import data, hip_ops
    root = data.write_synthetic_camels(str(tmp_path / "only256"), "CMD", fullsize=16, n_sims=4, seed=2)
    star = np.load(data.field_path(root, "CMD", "Astrid", "LH", "z_0.0", "Mstar"))
    np.save(data.field_path(root, "CMD", "Astrid", "LH", "z_0.0", "Mgas"), (3.0 * star[:, ::-1] + 1.0).astype(np.float32))
    np.save(data.field_path(root, "CMD", "Astrid", "LH", "z_0.0", "T"), (0.5 * star[:, :, ::-1] + 2.0).astype(np.float32))
    (tmp_path / "norm.json").write_text(json.dumps({"Mgas_m": 0.4, "Mgas_s": 0.25, "T_m": 0.5, "T_s": 0.1}))
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, str(tmp_path / "norm.json"))
    monkeypatch.setenv(data.DOWNGRID_ENV, "1")
    launches, real = [], hip_ops.augment_batch

    def counted(fields, *a, **k):
        launches.append(len(fields))
        return real(fields, *a, **k)
    monkeypatch.setattr(hip_ops, "augment_batch", counted)

    def first_batch(names):
        dm = data.get_dataset(dataset_name="CMD_128", return_func=data.cond_return_func(len(names) - 1), set_name="LH", channel_names=names,
                              stage="fit", batch_size=2, cropsize=4, data_root=root, seed=7)
        assert dm._derived_edge == [8] * len(names) and dm.fullsize == 8
        dm.device = DEV
        return dm, next(iter(dm.train_dataloader()))
    dm4, b4 = first_batch(["Mstar", "Mgas", "T", "Mcdm"])
    assert launches == [4] and b4["conditioning"].shape == (2, 3, 4, 4, 4) and b4["x"].shape == (2, 1, 4, 4, 4)
    assert len(dm4.state_dict()["norm"]) == 4 and [f.shape for f in dm4._dev_fields] == [(4, 8, 8, 8)] * 4
    for j, name in enumerate(["Mstar", "Mgas", "T"]):
        _, b2 = first_batch([name, "Mcdm"])
        assert torch.equal(b2["conditioning"], b4["conditioning"][:, j:j + 1]), name
        assert torch.equal(b2["x"], b4["x"])
    assert len({b4["conditioning"][:, j].sum().item() for j in range(3)}) == 3
