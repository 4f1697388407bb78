"""The flow-matching training step on the HIP backend through its fused head and loss (vdm_sfm_head / vdm_sfm_loss): against the chain of
generic launches it replaces (bit for bit), against the CPU oracle, captured in a hipGraph (trainer.GraphedTrainStep, Trainer.fit) and
resumed from a checkpoint.  Network: the one of tests/test_cond_fields_gpu.py (chs = (16, 32), 16^3, B = 2).
Tolerances: fused against unfused none (torch.equal); against oracle/sfm_oracle.py rel 2e-4, as tests/test_unet_gpu.py's SFM test; captured
against eager none, as test_graph_captured_step_equals_the_eager_step; resume none."""
import math

import pytest
import torch

import _resume_worker as W
from helpers import grf, oracle_cfg, oracle_params
from test_cond_fields_gpu import D, _reseed, make_net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 2


def make_sfm(net, **kw):
    from vdm4cdm_amd.sfm_model import LightSFM
    return LightSFM(velocity_model=net, draw_figure=None, learning_rate=3e-3, **kw)


def fields(seed=3):
    """(x0, x1, [v]) on the device: two distinct fields and one vector conditioning."""
    g = torch.Generator().manual_seed(seed + 2)
    return grf((B, 1, D, D, D), seed + 10).to(DEV), grf((B, 1, D, D, D), seed).to(DEV), [torch.rand(B, 6, generator=g).to(DEV)]


def loss_and_grad(sfm, fused, monkeypatch, **kw):
    import vdm4cdm_amd.sfm_model as sm
    monkeypatch.setattr(sm, "FUSED_HEAD", fused)
    _reseed(5)
    net = sfm.model.velocity_model
    x0, x1, v = fields()
    net.flat.grad = None
    loss, _ = sfm.model.get_loss(x0=x0, x1=x1, v_conditionings=v, **kw)
    loss.backward()
    return loss.detach().clone(), net.flat.grad.clone()


# =================================================================================================== fused against unfused
@pytest.mark.parametrize("K", [1, 0], ids=["cond", "nocond"])
@pytest.mark.parametrize("sigma", [0.0, 0.1])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fused_step_has_the_bits_of_the_chain(precision, sigma, K, monkeypatch):
    """Times and noise drawn (seeds reset in between): loss and, in fp32, every parameter gradient.  K = 0: a velocity network without a
    conditioning field (cond = 0: channel 1 of the packed input is zero, as pack_input writes it for a missing second field)."""
    from vdm4cdm_amd import hip_ops as ops
    sfm = make_sfm(make_net(K, precision=precision), sigma=sigma).to(DEV).train()
    calls, real = [], ops.sfm_head
    monkeypatch.setattr(ops, "sfm_head", lambda *a, **k: (calls.append(k.get("cond")), real(*a, **k))[1])
    lu, gu = loss_and_grad(sfm, False, monkeypatch)
    assert not calls
    lf, gf = loss_and_grad(sfm, True, monkeypatch)
    assert calls == [K]
    assert math.isfinite(lf.item()) and torch.equal(lf, lu), (lf.item(), lu.item())
    if precision == "fp32":
        net = sfm.model.velocity_model
        diff = [n for n in net.spec.items if not torch.equal(net.view(n, gf), net.view(n, gu))]
        assert gu.abs().max().item() > 0 and not diff, f"fused gradients differ from the chain's in {len(diff)} tensors: {diff[:8]}"


@pytest.mark.parametrize("sigma", [0.0, 0.1])
def test_fused_loss_matches_oracle(sigma, monkeypatch):
    """Supplied times and noise, fp32: the oracle's loss at the existing SFM test's tolerance."""
    import vdm4cdm_amd.sfm_model as sm
    from oracle import sfm_oracle, unet_oracle
    monkeypatch.setattr(sm, "FUSED_HEAD", True)
    net = make_net(1)
    sfm = make_sfm(net, sigma=sigma).to(DEV).train()
    x0, x1, v = fields()
    times, eps = torch.tensor([0.15, 0.65]), grf((B, 1, D, D, D), 21, slope=0.0)
    P = oracle_params(net)
    vel = lambda xt, t, x0_: unet_oracle.cunet_forward(P, oracle_cfg(net), xt, t, x0_, [a.cpu() for a in v])      # noqa: E731
    with torch.no_grad():
        ref, _, _ = sfm_oracle.sfm_loss(vel, x0.cpu(), x1.cpu(), times, eps=eps, sigma=sigma)
    loss, _ = sfm.model.get_loss(x0=x0, x1=x1, times=times.to(DEV), eps=eps.to(DEV), v_conditionings=v)
    assert loss.item() == pytest.approx(ref.item(), rel=2e-4)


def test_fused_step_launches_nothing_of_the_chain(monkeypatch):
    """diffuse, randn and pack_input raise while get_loss runs: the fused call (noise drawn in the kernel) forms its loss without them.
    (The network's own backward pass packs d loss / d v for conv_out's transposed conv with pack_input, fused or not: the patches are
    taken off before it runs.)"""
    import vdm4cdm_amd.sfm_model as sm
    from vdm4cdm_amd import hip_ops as ops
    monkeypatch.setattr(sm, "FUSED_HEAD", True)

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"the fused flow-matching step launched ops.{name}")
        return f
    sfm = make_sfm(make_net(1, precision="bf16"), sigma=0.1).to(DEV).train()
    x0, x1, v = fields()
    _reseed(5)
    with monkeypatch.context() as m:
        for name in ("diffuse", "randn", "pack_input"):
            m.setattr(ops, name, refuse(name))
        loss, _ = sfm.model.get_loss(x0=x0, x1=x1, v_conditionings=v)
    loss.backward()
    g = sfm.model.velocity_model.flat.grad
    assert math.isfinite(loss.item()) and torch.isfinite(g).all() and g.abs().max().item() > 0


# =================================================================================================== captured step
def test_captured_step_equals_the_eager_step(monkeypatch):
    """bf16, dropout on, sigma = 0.1: three replays of GraphedTrainStep against three eager steps with the same baked host seeds and the
    device step counter bound the same way - losses, clipped gradients and parameters after every step, bit for bit; the network times
    come from the device counter and differ from replay to replay."""
    from vdm4cdm_amd import hip_ops as ops
    from vdm4cdm_amd.trainer import GraphedTrainStep, clip_grad_norm_flat_, rng_state, set_rng_state
    seen, real = [], ops.train_scalars
    monkeypatch.setattr(ops, "train_scalars", lambda *a, **k: (seen.append(real(*a, **k)), seen[-1])[1])     # (the reference keeps the block)
    x0, x1, v = fields()
    batch = {"x0": x0, "x1": x1, "conditioning_values": v}

    def build():
        sfm = make_sfm(make_net(1, precision="bf16", dropout=0.1, seed=8), sigma=0.1).to(DEV).train()
        params = [p for p in sfm.parameters() if p.requires_grad]
        _reseed(5)
        sfm.model._graph_seed = 1234
        return sfm, params, sfm.configure_optimizers(capturable=True)

    # eager: the constructor's three warm-up steps draw three sets of host seeds, the capture bakes the fourth into every replay
    sfm, params, opt = build()
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    eager = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    try:
        ops.SEED_STEP = counter
        with torch.cuda.stream(side):
            with torch.no_grad():
                for _ in range(3):
                    sfm.training_step(batch, 0)
            baked = rng_state(sfm, DEV)
            for step in range(3):
                set_rng_state(sfm, DEV, baked)
                loss = sfm.training_step(batch, 0)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                clip_grad_norm_flat_(params, 0.5, True, want_norm=True)
                opt.step()
                ops.step_inc(counter)
                eager.append((loss.detach().clone(), params[0].grad.clone(), params[0].detach().clone(), seen[-1][0].clone()))
                del loss
    finally:
        ops.SEED_STEP = None
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert counter.item() == 3

    sfm, params, opt = build()
    del seen[:]
    gs = GraphedTrainStep(sfm, opt, params, 0.5, batch)
    assert len(seen) == 4 and ops.SEED_STEP is None                  # three warm-up steps and the capture
    t_static = seen[-1][0]
    ts = []
    for step, (le, ge, pe, te) in enumerate(eager):
        lg = gs(batch)
        torch.cuda.synchronize()
        ts.append(t_static.clone())
        assert torch.isfinite(ge).all() and torch.equal(le, lg), (step, le.item(), lg.item())
        assert torch.equal(ts[-1], te), (step, ts[-1].tolist(), te.tolist())
        net = sfm.model.velocity_model
        diff = [n for n in net.spec.items if not torch.equal(net.view(n, ge), net.view(n, params[0].grad))]
        assert not diff, f"step {step}: captured step differs from the eager step in {len(diff)} gradient tensors: {diff[:8]}"
        assert torch.equal(pe, params[0].detach()), f"step {step}: parameters differ"
    assert gs.counter.item() == 3 and len(seen) == 4
    assert not torch.equal(ts[0], ts[1]) and not torch.equal(ts[1], ts[2])
    assert not torch.equal(eager[0][0], eager[1][0])
    del gs


# =================================================================================================== Trainer.fit
def sfm_batch(fields_, params):
    return {"x0": fields_[0], "x1": fields_[1], "conditioning_values": [params]}


def run_fit(root, name, max_steps, every, graph=True, ckpt_path=None, **sfm_kw):
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    from vdm4cdm_amd.trainer import Trainer
    W.fresh_process()
    sfm = make_sfm(make_net(1, precision="bf16", dropout=0.1, seed=21), sigma=0.1, **sfm_kw)
    dm = SyntheticAstroDataModule(cropsize=D, batch_size=B, n_train=8, n_val=4, seed=5, return_func=sfm_batch)
    tr = Trainer(max_steps=max_steps, val_check_interval=0, gradient_clip_val=0.5, every_n_train_steps=every, default_root_dir=str(root),
                 experiment_name=name, device="cuda", enable_progress=False, log_every_n_steps=1, graph_step=graph)
    tr.fit(sfm, dm, **({} if ckpt_path is None else {"ckpt_path": ckpt_path}))
    return tr, sfm


def test_fit_trains_from_a_captured_step(tmp_path, capsys):
    tr, _ = run_fit(tmp_path, "g", 10, 0)
    assert tr.graphed_step is not None and tr.graphed_step.replays == 10 and tr.global_step == 10
    losses = W.losses(tr.history)
    assert losses.numel() == 10 and torch.isfinite(losses).all() and losses.unique().numel() == 10
    assert "stays eager" not in capsys.readouterr().out


def test_fit_stays_eager_without_antithetic_times(tmp_path, capsys):
    tr, _ = run_fit(tmp_path, "e", 10, 0, antithetic_time_sampling=False)
    out = capsys.readouterr().out
    assert tr.graphed_step is None and tr.global_step == 10 and torch.isfinite(W.losses(tr.history)).all()
    assert out.count("the training step stays eager") == 1 and "antithetic_time_sampling=False" in out


def test_sfm_training_script_entry_trains_from_a_captured_step(tmp_path, monkeypatch):
    """What trainSFM3D128_c_c_from_field_name_thick_lowbatch.py runs (entry.train_sfm3d) with VDM4CDM_GRAPH_STEP=1 on a synthetic
    on-disk data set: the file-backed data module's {"x0", "x1", "conditioning_values"} batches feed a captured step."""
    import json
    from vdm4cdm_amd import data, entry
    root = data.write_synthetic_camels(str(tmp_path / "camels"), dataset_name="CMD_128", n_sims=9, fullsize=16, seed=1)
    for k, v in dict(VDM4CDM_GRAPH_STEP="1", VDM4CDM_MAX_STEPS="10", VDM4CDM_LOG_DIR=str(tmp_path), VDM4CDM_PRECISION="bf16",
                     VDM4CDM_DATA_ROOT=root).items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("VDM4CDM_RESUME", raising=False)
    tr = entry.train_sfm3d("128", ["Mstar", "Mcdm", "16"])
    assert tr.global_step == 10 and tr.graphed_step is not None and tr.graphed_step.replays >= 8
    with open(tmp_path / "LH128_c_c_Mstar_to_Mcdm_thick_lowbatch_16" / "metrics.jsonl") as f:
        recs = [json.loads(line) for line in f]
    assert recs and all("train/loss" in r and math.isfinite(r["loss"]) for r in recs)


def test_graphed_resume_is_bitwise_the_uninterrupted_run(tmp_path):
    """Six graphed steps against three, a checkpoint and three more.  A step is captured only in a run with at least 8 steps ahead of it,
    so the uninterrupted run has max_steps = 8 and is compared at its checkpoint of step 6; the continuation of its checkpoint of step 3
    stops at max_steps = 6.  A graphed checkpoint continued eagerly is refused."""
    from vdm4cdm_amd.trainer import read_checkpoint
    tr_a, _ = run_fit(tmp_path, "a", 8, 3)
    assert tr_a.graphed_step is not None and tr_a.graphed_step.replays == 8
    a = read_checkpoint(W.ckpt_at(tmp_path, "a", 6))
    assert a["trainer_state"]["graph"]["counter"] == 6
    tr_b, sfm_b = run_fit(tmp_path, "b", 6, 0, ckpt_path=W.ckpt_at(tmp_path, "a", 3))
    assert tr_b.graphed_step is not None and tr_b.graphed_step.replays == 3 and tr_b.global_step == 6
    sd = sfm_b.state_dict()
    assert sorted(sd) == sorted(a["state_dict"])
    bad = [k for k in sd if not torch.equal(sd[k].cpu(), a["state_dict"][k])]
    assert not bad, f"parameters differ: {bad[:8]}"
    sa, sb = a["trainer_state"]["optimizer"]["state"], tr_b.optimizers[0].state_dict()["state"]
    assert sorted(sa) == sorted(sb) and len(sa) >= 1
    for i in sa:
        assert sorted(sa[i]) == sorted(sb[i]) and {"exp_avg", "exp_avg_sq", "step"} <= set(sa[i])
        for k in sa[i]:
            assert torch.equal(torch.as_tensor(sa[i][k]).cpu(), torch.as_tensor(sb[i][k]).cpu()), f"optimizer state {i}.{k} differs"
    la = torch.tensor([h["loss"] for h in tr_a.history if 3 < h["step"] <= 6], dtype=torch.float64)
    lb = W.losses(tr_b.history, 3)
    assert la.numel() == 3 and torch.equal(la, lb), (la.tolist(), lb.tolist())
    with pytest.raises(ValueError, match="graph-captured training step"):
        run_fit(tmp_path, "c", 6, 0, graph=False, ckpt_path=W.ckpt_at(tmp_path, "a", 3))
