"""Conditioning dropout for classifier-free guidance on the HIP backend: a training step with p_uncond = 0.5 is, bit for bit, the step
of a p_uncond = 0 model fed the inputs the host masked with last_cond_keep (fused head, unfused head, learned schedule; input
gradients; the graph-captured step, replay by replay; stop and resume), and the guided samplers with cfg_drop "s" / "vs".

Network: that of tests/test_cond_fields_gpu.py (make_net: 16^3, chs (16, 32), dropout 0), batch 4.  SEED is one whose first mask of
four rows holds a kept and a dropped row and whose first six masks differ; the tests assert that before they rely on it."""
import numpy as np
import pytest
import torch

from _cfg_ref import keep_rows
from helpers import grf
from test_cond_fields_gpu import DEV, inputs, make_net, make_vdm

pytestmark = pytest.mark.gpu
SEED, B, P = 20240611, 4, 0.5


def _reseed(seed=SEED):
    import vdm4cdm_amd.unet_hip as uh
    import vdm4cdm_amd.vdm_model as vm
    torch.manual_seed(seed)
    uh._seed_counter[0] = 0
    vm.reset_train_generators()


def _where(t, keep):
    """Host-side masking of the rows (a select: +0 in the dropped rows)."""
    k = keep.to(t.device).view((-1,) + (1,) * (t.dim() - 1))
    return torch.where(k != 0, t, torch.zeros_like(t))


def _mask(s, v, keep, drop):
    return (_where(s, keep) if "s" in drop else s), ([_where(a, keep) for a in v] if "v" in drop else v)


def _model(K, precision, path, **kw):
    sched = dict(noise_schedule="learned_linear", gamma_min=-13.3) if path == "learned" else {}
    return make_vdm(make_net(K, precision=precision), **sched, **kw).to(DEV).train()


def _step(vdm, x, s, v, path, grads=False):
    """One training step from the fixed generator state; (loss, flat grad, schedule grads or None, input grads or None)."""
    _reseed()
    sd, vd = s.to(DEV).requires_grad_(grads), [a.to(DEV).requires_grad_(grads) for a in v]
    kw = dict(s_conditioning=sd, v_conditionings=vd)
    if path == "unfused":
        kw.update(eps=grf(x.shape, 50, slope=0.0).to(DEV), eps0=grf(x.shape, 51, slope=0.0).to(DEV))
    vdm.zero_grad(set_to_none=True)
    loss, _ = vdm.model.get_loss(x.to(DEV), **kw)
    loss.backward()
    m = vdm.model
    sched = (m.gamma_b.grad.clone(), m.gamma_w.grad.clone()) if path == "learned" else None
    return loss.detach().clone(), m.score_model.flat.grad.clone(), sched, ((sd.grad, [a.grad for a in vd]) if grads else None)


def _expected_keep(vdm, step=0, rows=B):
    return keep_rows(vdm.model.cond_keep_seed, P, 0, rows, step=step)


# ------------------------------------------------------------------------------------------ equivalence
@pytest.mark.parametrize("path", ["fused", "unfused", "learned"])
@pytest.mark.parametrize("drop", ["v", "s", "vs"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("K", [1, 3])
def test_training_step_equals_the_step_on_host_masked_inputs(K, precision, drop, path):
    _reseed()
    a = _model(K, precision, path, p_uncond=P, cfg_drop=drop)
    want = _expected_keep(a)
    assert set(want.tolist()) == {0.0, 1.0}, f"seed {SEED}: the first mask {want} does not hold both a kept and a dropped row"
    x, _, s, v = inputs(a.model.score_model, B)
    la, ga, sa, _ = _step(a, x, s, v, path)
    keep = a.model.last_cond_keep
    assert keep.is_cuda and keep.dtype == torch.float32 and np.array_equal(keep.cpu().numpy(), want), (keep, want)
    b = _model(K, precision, path)
    assert torch.equal(a.model.score_model.flat, b.model.score_model.flat)
    sm, vm_ = _mask(s, v, keep.cpu(), drop)
    lb, gb, sb, _ = _step(b, x, sm, vm_, path)
    assert b.model.last_cond_keep is None
    lc, _, _, _ = _step(b, x, s, v, path)
    assert not torch.equal(la, lc), "the masked and the unmasked step have the same loss: the comparison would show nothing"
    assert torch.isfinite(ga).all() and torch.equal(la, lb), (la.item(), lb.item())
    assert torch.equal(ga, gb), f"{(ga != gb).sum().item()} of {ga.numel()} parameter gradients differ"
    if path == "learned":
        assert torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1]) and sa[0].item() != 0.0 and sa[1].item() != 0.0
    # the next eager step draws the next mask (host call counter)
    _step(a, x, s, v, path)
    assert np.array_equal(a.model.last_cond_keep.cpu().numpy(), _expected_keep(a, step=1))


@pytest.mark.parametrize("K", [1, 3])
def test_input_gradients_of_dropped_rows_are_zero(K):
    """Learned schedule, v and s require grad, cfg_drop "vs": dropped rows get exactly-zero gradients, kept rows the bits of the
    masked-input run."""
    _reseed()
    a = _model(K, "fp32", "learned", p_uncond=P, cfg_drop="vs")
    x, _, s, v = inputs(a.model.score_model, B)
    _, _, _, (dsa, dva) = _step(a, x, s, v, "learned", grads=True)
    keep = a.model.last_cond_keep.cpu()
    assert set(keep.tolist()) == {0.0, 1.0}
    b = _model(K, "fp32", "learned")
    sm, vm_ = _mask(s, v, keep, "vs")
    _, _, _, (dsb, dvb) = _step(b, x, sm, vm_, "learned", grads=True)
    kept, dropped = keep != 0, keep == 0
    for what, ga, gb in [("ds", dsa, dsb)] + [(f"dv[{j}]", p, q) for j, (p, q) in enumerate(zip(dva, dvb))]:
        ga, gb = ga.cpu(), gb.cpu()
        assert ga.shape[0] == B and torch.isfinite(ga).all() and gb[dropped].abs().max().item() > 0, what   # (the p = 0 run has them)
        assert torch.equal(ga[dropped].contiguous().view(torch.uint8), torch.zeros_like(ga[dropped]).view(torch.uint8)), f"{what}: dropped rows"
        assert torch.equal(ga[kept], gb[kept]) and ga[kept].abs().max().item() > 0, f"{what}: kept rows"


# ------------------------------------------------------------------------------------------ captured step
@pytest.mark.parametrize("drop", ["vs"])
def test_captured_step_draws_a_fresh_mask_per_replay(drop):
    """GraphedTrainStep, six replays (learning rate 0: the weights stay, so that every replay can be compared with an eager step): after
    replay i last_cond_keep is the reference mask of step i, and the loss is the loss of the eager p_uncond = 0 step on the batch the
    host masked - with the same baked seeds and device counter, bit for bit (what tests/test_unet_gpu.py asserts of graphed vs eager)."""
    import vdm4cdm_amd.unet_hip as uh
    import vdm4cdm_amd.vdm_model as vm
    from vdm4cdm_amd import hip_ops as ops
    from vdm4cdm_amd.trainer import GraphedTrainStep
    K, n = 3, 6
    try:
        _reseed()
        a = make_vdm(make_net(K), p_uncond=P, cfg_drop=drop).to(DEV).train()
        a.learning_rate = 0.0
        masks = [_expected_keep(a, step=i) for i in range(n)]
        assert any(not np.array_equal(masks[0], m) for m in masks[1:]), "the first six masks are all equal"
        x, _, s, v = inputs(a.model.score_model, B)
        batch = lambda s_, v_: {"x": x.to(DEV), "conditioning": s_.to(DEV), "conditioning_values": [t.to(DEV) for t in v_]}
        params = [p for p in a.parameters() if p.requires_grad]
        gs = GraphedTrainStep(a, a.configure_optimizers(capturable=True), params, 0.5, batch(s, v))
        losses = []
        for i in range(n):
            losses.append(gs(batch(s, v)).detach().clone())
            torch.cuda.synchronize()
            assert np.array_equal(a.model.last_cond_keep.cpu().numpy(), masks[i]), (i, a.model.last_cond_keep, masks[i])
        assert gs.counter.item() == n and a.rng_state_dict().get("cond_keep_calls") is None      # (the host counter is the eager steps')
        del gs
        # the eager reference: the same generator history (3 warm-up steps, then the step whose seeds the graph baked in)
        _reseed()
        b = make_vdm(make_net(K)).to(DEV).train()
        counter = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.SEED_STEP = counter
        for _ in range(3):
            b.training_step(batch(s, v), 0)
        snap, drop_ctr = vm.train_generator_states(), uh._seed_counter[0]
        for i in range(n):
            vm.set_train_generator_states(snap)
            uh._seed_counter[0] = drop_ctr
            counter.fill_(i)
            sm, vm_ = _mask(s, v, torch.from_numpy(masks[i]), drop)
            le = b.training_step(batch(sm, vm_), 0).detach()
            assert torch.equal(le, losses[i]), (i, le.item(), losses[i].item())
        assert len({float(l) for l in losses}) == n
    finally:
        ops.SEED_STEP = None


# ------------------------------------------------------------------------------------------ resume
def test_resume_with_conditioning_dropout_is_bitwise_the_uninterrupted_run(tmp_path, monkeypatch):
    """In the manner of tests/test_resume_gpu.py (its worker's network, data and comparison; the model gets p_uncond = 0.5): 12 eager
    steps against 6 steps + checkpoint + 6 resumed steps; resuming with another p_uncond raises."""
    import _resume_worker as W
    made = W.make_model
    conf = {"p": P}

    def make_model(**kw):
        vdm = made(**kw)
        vdm.model.p_uncond, vdm.model.cfg_drop = conf["p"], "vs"
        return vdm
    monkeypatch.setattr(W, "make_model", make_model)
    kw = dict(device="cuda", model_kw=dict(backend="hip", precision="fp32"))
    a = W.run_fit(tmp_path, "a", 12, 0, **kw)
    W.run_fit(tmp_path, "b", 6, 6, **kw)
    path = W.ckpt_at(tmp_path, "b", 6)
    ck = torch.load(path, map_location="cpu")
    assert ck["cfg_dropout"] == {"p_uncond": P, "cfg_drop": "vs"} and ck["trainer_state"]["rng"]["model"]["cond_keep_calls"] == 6
    b = W.run_fit(tmp_path, "b", 12, 0, ckpt_path=path, **kw)
    W.assert_same_run(a, b, 6, 12)
    conf["p"] = 0.0                                                       # the feature matters to this run
    c = W.run_fit(tmp_path, "c", 12, 0, **kw)
    assert not torch.equal(a["flat"], c["flat"])
    conf["p"] = 0.25
    with pytest.raises(ValueError, match="p_uncond"):
        W.run_fit(tmp_path, "b", 12, 0, ckpt_path=path, **kw)


# ------------------------------------------------------------------------------------------ guided sampling
def _guided(drop, K=2, w=1.5):
    net = make_net(K)
    vdm = make_vdm(net, w_cfg=w, cfg_drop=drop).to(DEV).eval()
    x, _, s, v = inputs(net, 2)
    return net, vdm, x.to(DEV), s.to(DEV), [a.to(DEV) for a in v]


@pytest.mark.parametrize("drop", ["s", "vs"])
def test_unguided_half_masks_what_cfg_drop_names(drop):
    """get_pred_noise under w_cfg = 1.5 is (1 + w) net(z, s, v) - w net(z, 0, v or 0) of separate forwards (bound of
    test_classifier_free_guidance_is_the_blend_of_two_forwards: the conv plans differ with the batch size)."""
    w = 1.5
    net, vdm, xd, sd, vd = _guided(drop, w=w)
    with torch.no_grad():
        g_t = vdm.model.gamma(torch.tensor(0.6, device=DEV))
        e = vdm.model.get_pred_noise(xd, g_t, s_conditioning=sd, v_conditionings=vd)
        tn = ((g_t + 13.3) / 26.6).expand(2)
        e_c = net(xd, t=tn, s_conditioning=sd, v_conditionings=vd)
        e_u = net(xd, t=tn, s_conditioning=torch.zeros_like(sd), v_conditionings=vdm.model.cfg_mask(vd) if "v" in drop else vd)
        e_o = net(xd, t=tn, s_conditioning=torch.zeros_like(sd), v_conditionings=vd if "v" in drop else vdm.model.cfg_mask(vd))
    blend, other = (1.0 + w) * e_c - w * e_u, (1.0 + w) * e_c - w * e_o
    tol = 1e-4 * blend.abs().max().item() + 1e-5
    assert (blend - other).abs().max().item() > 10 * tol, "masking v makes no difference: 's' and 'vs' could not be told apart"
    assert (e - blend).abs().max().item() <= tol


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("sampler", ["ancestral", "dpm2m"])
@pytest.mark.parametrize("drop", ["s", "vs"])
def test_guided_sampler_matches_the_eager_product_loop(drop, sampler, use_graph):
    """w_cfg = 1.5, 4 steps: the device loop (NetStep: zero planes concatenated once) against the Python loop over get_pred_noise
    (VDM._cfg_pair) fed the same z_1 and noises.  Bound: 2e-3 max|eager|, as test_cfg_on_the_graph_path_matches_the_eager_product_loop."""
    from vdm4cdm_amd.sampling import multistep_loop
    n = 4
    net, vdm, xd, sd, vd = _guided(drop)
    m, kw = vdm.model, dict(s_conditioning=sd, v_conditionings=vd)
    z1 = grf(tuple(xd.shape), 60, slope=0.0).to(DEV)
    noises = [grf(tuple(xd.shape), 100 + i, slope=0.0).to(DEV) for i in range(n)]
    steps = torch.linspace(1.0, 0.0, n + 1, device=DEV)
    with torch.no_grad():
        if sampler == "ancestral":
            out = vdm.draw_samples(batch_size=2, n_sampling_steps=n, z=z1.clone(), noises=noises, use_graph=use_graph, **kw)
            z = z1.clone()
            for i in range(n):
                w_z, w_x, x0, scale = m.sample_zs_given_zt(zt=z, t=steps[i], s=steps[i + 1], return_ddnm=True, **kw)
                z = w_z * z + w_x * x0 + scale * noises[i]
        else:
            out = vdm.draw_samples(batch_size=2, n_sampling_steps=n, z=z1.clone(), sampler=sampler, use_graph=use_graph, **kw)
            coef = m.multistep_table(n, 2, True)
            z = multistep_loop(coef, z1.clone(), lambda i, zt: m.get_pred_noise(zt=zt, gamma_t=m.gamma(steps[i]), **kw), False)
        plain = make_vdm(net).to(DEV).eval().draw_samples(batch_size=2, n_sampling_steps=n, z=z1.clone(), sampler=sampler,
                                                          **({"noises": noises} if sampler == "ancestral" else {}), **kw)
    top = z.abs().max().item()
    err = (out - z).abs().max().item()
    print(f"{drop} {sampler} graph={use_graph}: err {err:.3e} (bound {2e-3 * top:.3e})")
    assert (z - plain).abs().max().item() > 1e-2 * top, "guidance does not move this chain: the test would show nothing"
    assert torch.isfinite(out).all() and err <= 2e-3 * top


def test_cfg_drop_v_is_the_pair_of_before():
    """cfg_drop "v" (the default): _cfg_pair is the batch-doubled forward on (v, cfg_mask(v)) with the field in both halves - the bits
    of that forward; the sampler equals the default-constructed model's."""
    net, vdm, xd, sd, vd = _guided("v")
    m = vdm.model
    with torch.no_grad():
        t = torch.full((2,), 0.6, device=DEV)
        e_c, e_u = m._cfg_pair(xd, t, dict(s_conditioning=sd, v_conditionings=vd))
        both = net(torch.cat([xd, xd]), t=torch.cat([t, t]), s_conditioning=torch.cat([sd, sd]),
                   v_conditionings=[torch.cat([a, z]) for a, z in zip(vd, m.cfg_mask(vd))])
        assert torch.equal(e_c, both[:2]) and torch.equal(e_u, both[2:])
        kw = dict(batch_size=2, n_sampling_steps=4, seeds=[1, 2], s_conditioning=sd, v_conditionings=vd)
        default = make_vdm(net, w_cfg=1.5).to(DEV).eval()
        assert default.model.cfg_drop == "v" and torch.equal(vdm.draw_samples(**kw), default.draw_samples(**kw))
