"""Exponential moving average of the weights on the HIP backend, model level: the eager and the graph-captured step average into the
shadows exactly as tests/_ema_ref.py says and leave training untouched, bit for bit; the warm-up steps of the captured step leave no
trace; evaluation under ema_weights() and what it restores; graphed resume; flow matching; the learned-schedule scalars.
Network and data: the smallest of the suite (16^3, two levels, batch 2, dropout on; tests/_ema_ref.py)."""
import numpy as np
import pytest
import torch

import _ema_ref as R
import _resume_worker as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DECAY = 0.5


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def hip_vdm(**kw):
    return lambda: R.make_vdm(backend="hip", precision="bf16", **kw)


def same_training(on, off):
    assert len(on["params"]) == len(off["params"])
    for i, (a, b) in enumerate(zip(on["params"], off["params"])):
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y)), f"raw parameters differ after step {i}"
    la, lb = W.losses(on["history"]), W.losses(off["history"])
    assert la.numel() > 0 and torch.equal(la, lb)


@pytest.fixture
def count_updates(monkeypatch):
    from vdm4cdm_amd import hip_ops as ops
    calls, orig = [], ops.ema_update

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    monkeypatch.setattr(ops, "ema_update", counted)
    return calls


def test_eager_step_averages_and_does_not_perturb_training(tmp_path, count_updates):
    on = R.run_fit(tmp_path, "on", hip_vdm(ema_decay=DECAY), 6, device="cuda")
    assert len(count_updates) == 6 and on["trainer"].graphed_step is None
    off = R.run_fit(tmp_path, "off", hip_vdm(), 6, device="cuda")
    assert len(count_updates) == 6 and off["model"].ema is None                 # EMA off: the entry is never called
    same_training(on, off)
    assert on["model"].ema.hip and on["model"].ema.counter.dtype == torch.int32 and on["model"].ema.counter.is_cuda
    R.assert_shadows_follow_ref(on, DECAY, True)
    assert not np.array_equal(on["shadows"][0], on["params"][-1][0])


def test_graphed_step_averages_and_its_warmup_leaves_no_trace(tmp_path, count_updates):
    """10 steps with graph_step=True: the three eager warm-up steps of the capture update the shadows and bump the counter, and both
    are put back - the counter ends at the number of real steps and the shadow is the reference over the real steps' parameters."""
    on = R.run_fit(tmp_path, "on", hip_vdm(ema_decay=DECAY), 10, device="cuda", graph=True)
    assert on["trainer"].graphed_step is not None and on["trainer"].graphed_step.replays == 10
    assert len(count_updates) == 4                                            # three warm-up steps and the capture; replays call nothing
    off = R.run_fit(tmp_path, "off", hip_vdm(), 10, device="cuda", graph=True)
    assert len(count_updates) == 4 and off["trainer"].graphed_step.replays == 10
    same_training(on, off)
    assert on["num_updates"] == 10
    R.assert_shadows_follow_ref(on, DECAY, True)


def test_graphed_resume_is_the_uninterrupted_run(tmp_path):
    mk = hip_vdm(ema_decay=DECAY)
    a = R.run_fit(tmp_path, "a", mk, 10, device="cuda", graph=True)
    b1 = R.run_fit(tmp_path, "b", mk, 10, device="cuda", graph=True, every=5)
    b = R.run_fit(tmp_path, "b", mk, 10, device="cuda", graph=True, ckpt_path=W.ckpt_at(tmp_path, "b", 5))
    ck = torch.load(W.ckpt_at(tmp_path, "b", 5), map_location="cpu")
    assert ck["ema"] == {"decay": DECAY, "warmup": True, "num_updates": 5} and ck["trainer_state"]["graph"]["counter"] == 5
    assert b["trainer"].graphed_step.replays == 5 and len(b["params"]) == 6
    for run in (b1, b):
        assert run["num_updates"] == a["num_updates"] == 10
        for x, y in zip(run["shadows"] + run["params"][-1], a["shadows"] + a["params"][-1]):
            assert np.array_equal(bits(x), bits(y))
    assert torch.equal(W.losses(a["history"], 5), W.losses(b["history"], 5))


def _batch():
    b = next(iter(R.make_dm().train_dataloader()))
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in b.items()}


def _samples_raw(vdm, ck, skw):
    """The samples of a model that loaded the checkpoint's RAW weights."""
    raw = R.make_vdm(backend="hip", precision="bf16")
    raw.load_state_dict(ck["state_dict"])
    return raw.to(DEV).eval().draw_samples(**skw)


def test_ema_weights_context_samples_from_the_average_and_restores_every_bit(tmp_path):
    run = R.run_fit(tmp_path, "on", hip_vdm(ema_decay=DECAY), 6, device="cuda", every=6)
    vdm, ema = run["model"], run["model"].ema
    net = vdm.model.score_model
    batch = _batch()
    x, kw = vdm._unpack(batch)
    t = torch.tensor([0.3, 0.7], device=DEV)
    vdm.eval()
    with torch.no_grad():
        y_raw = net(x, t=t, **kw).clone()
    flat_raw, shadow = net.flat.detach().clone(), ema.shadows[0].clone()
    # a second model that loaded the checkpoint's averaged weights
    ck = torch.load(W.ckpt_at(tmp_path, "on", 6), map_location="cpu")
    other = R.make_vdm(backend="hip", precision="bf16")
    other.load_state_dict(ck["ema_state_dict"])
    other.to(DEV).eval()
    assert torch.equal(other.model.score_model.flat.detach(), shadow)
    skw = dict(batch_size=2, n_sampling_steps=4, seed=11, **kw)
    want = other.draw_samples(**skw)
    with torch.no_grad():
        y_ema = other.model.score_model(x, t=t, **kw).clone()
    with vdm.ema_weights():
        assert torch.equal(net.flat.detach(), shadow) and torch.equal(ema.shadows[0], flat_raw)
        got = vdm.draw_samples(**skw)
        with torch.no_grad():
            assert torch.equal(net(x, t=t, **kw), y_ema)
        with pytest.raises(RuntimeError, match="re-entrant"):
            with vdm.ema_weights():
                pass
    assert torch.equal(got, want) and not torch.equal(y_ema, y_raw)
    assert torch.equal(net.flat.detach(), flat_raw) and torch.equal(ema.shadows[0], shadow) and ema.num_updates == 6
    with torch.no_grad():
        assert torch.equal(net(x, t=t, **kw), y_raw)
    assert torch.equal(vdm.draw_samples(**skw), _samples_raw(vdm, ck, skw))


def test_graphed_step_replays_the_same_after_the_context():
    """Two identical captured steps, three replays each; one enters ema_weights() (and runs a forward pass in it) before the third:
    the third replay's loss, the parameters and the shadows have the same bits in both."""
    from vdm4cdm_amd.trainer import GraphedTrainStep
    batch = _batch()

    def run(enter):
        W.fresh_process()
        vdm = R.make_vdm(backend="hip", precision="bf16", ema_decay=DECAY).to(DEV).train()
        params = [p for p in vdm.parameters() if p.requires_grad]
        opt = vdm.configure_optimizers(capturable=True)
        gs = GraphedTrainStep(vdm, opt, params, 0.5, batch)
        assert vdm.ema.num_updates == 0 and torch.equal(vdm.ema.shadows[0], params[0].detach())
        losses = [float(gs(batch)) for _ in range(2)]
        if enter:
            x, kw = vdm._unpack(batch)
            with vdm.ema_weights(), torch.no_grad():
                vdm.eval()
                vdm.model.score_model(x, t=torch.tensor([0.3, 0.7], device=DEV), **kw)
                vdm.train()
        losses.append(float(gs(batch)))
        torch.cuda.synchronize()
        return losses, params[0].detach().clone(), vdm.ema.shadows[0].clone(), vdm.ema.num_updates

    a, b = run(False), run(True)
    assert a[0] == b[0] and len(set(a[0])) == 3
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] == 3


def test_validation_inside_a_graphed_fit_leaves_training_alone(tmp_path):
    on = R.run_fit(tmp_path, "on", hip_vdm(ema_decay=DECAY), 10, device="cuda", graph=True, val=5)
    off = R.run_fit(tmp_path, "off", hip_vdm(), 10, device="cuda", graph=True, val=5)
    same_training(on, off)
    R.assert_shadows_follow_ref(on, DECAY, True)
    assert on["trainer"].graphed_step.replays == 10
    v_on, v_off = W.losses(on["history"], key="val_loss"), W.losses(off["history"], key="val_loss")
    assert v_on.numel() == 2 and not torch.equal(v_on, v_off)                  # (the validation loss is the averaged weights')


def test_flow_matching_eager_step_averages(tmp_path):
    mk = lambda **kw: (lambda: R.make_sfm(backend="hip", precision="bf16", **kw))
    on = R.run_fit(tmp_path, "on", mk(ema_decay=DECAY), 6, device="cuda", sfm=True, every=6)
    off = R.run_fit(tmp_path, "off", mk(), 6, device="cuda", sfm=True)
    same_training(on, off)
    R.assert_shadows_follow_ref(on, DECAY, True)
    ck = torch.load(W.ckpt_at(tmp_path, "on", 6), map_location="cpu")
    assert set(ck["ema_state_dict"]) == set(ck["state_dict"]) and all(k.startswith("model.velocity_model.") for k in ck["ema_state_dict"])


def test_learned_schedule_scalars_follow_the_reference(tmp_path):
    """gamma_b / gamma_w go through vdm_ema_update with n = 1 (the scalar path, whatever their alignment)."""
    on = R.run_fit(tmp_path, "on", hip_vdm(schedule="learned_linear", ema_decay=DECAY), 6, device="cuda")
    off = R.run_fit(tmp_path, "off", hip_vdm(schedule="learned_linear"), 6, device="cuda")
    same_training(on, off)
    assert [s.size for s in on["shadows"]][1:] == [1, 1]
    R.assert_shadows_follow_ref(on, DECAY, True)
    assert all(not np.array_equal(s, p) for s, p in zip(on["shadows"], on["params"][-1]))
