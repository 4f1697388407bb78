"""Resumable training on the HIP backend: a fit stopped at step K and continued from its checkpoint by fresh objects is the
uninterrupted fit BIT FOR BIT (parameters, every optimizer-state tensor, logged losses; no tolerance) - eager step in fp32 and bf16
storage, learned-linear schedule, graph-captured step - and GraphedTrainStep puts a non-empty optimizer state back after its warm-up.
Network and data: tests/_resume_worker.py (16^3, two levels, batch 2, dropout 0.1 on: the dropout seed stream is part of the state)."""
import pytest
import torch

import _resume_worker as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _stop_and_resume(tmp_path, N, K, graph=False, **model_kw):
    kw = dict(device="cuda", graph=graph, model_kw=dict(backend="hip", **model_kw))
    a = W.run_fit(tmp_path, "a", N, 0, **kw)
    # the interrupted run is the SAME run (max_steps = N decides whether the step is captured), used up to its checkpoint at K
    b1 = W.run_fit(tmp_path, "b", N if graph else K, K, **kw)
    b = W.run_fit(tmp_path, "b", N, 0, ckpt_path=W.ckpt_at(tmp_path, "b", K), **kw)
    W.assert_same_run(a, b, K, N)
    assert float(b["opt"]["0.step"]) == N and b["history"][0]["step"] == K + 1 and "resumed_from" in b["history"][0]
    return a, b1, b


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_resume_is_bitwise_the_uninterrupted_run_eager(tmp_path, precision):
    a, b1, b = _stop_and_resume(tmp_path, 8, 3, precision=precision)
    assert b["replays"] is None and not torch.equal(b1["flat"], b["flat"])
    ts = torch.load(W.ckpt_at(tmp_path, "b", 3), map_location="cpu")["trainer_state"]
    assert ts["rng"]["dropout_seed_counter"] > 0 and "torch_device" in ts["rng"] and ts["graph"] is None


def test_resume_is_bitwise_the_uninterrupted_run_learned_schedule(tmp_path):
    """gamma_b / gamma_w travel in state_dict, their moments with the optimizer (the model's first two parameters: values 0 and 1 of
    the flat comparison, optimizer-state entries 0.* and 1.*)."""
    a, b1, b = _stop_and_resume(tmp_path, 8, 3, precision="bf16", schedule="learned_linear")
    assert {"0.exp_avg", "1.exp_avg_sq", "2.exp_avg"} <= set(b["opt"]) and b["opt"]["0.exp_avg"].numel() == 1
    assert b["opt"]["0.exp_avg"].abs().item() > 0 and b["opt"]["1.exp_avg"].abs().item() > 0
    assert (a["flat"][:2] != b1["flat"][:2]).all()               # the schedule moved between K and N


def test_resume_is_bitwise_the_uninterrupted_run_graphed(tmp_path):
    """graph_step=True, N = 12, K = 5 (4 batches per epoch).  The checkpoint keeps the generator states of immediately before the
    capture and the device counter; the resumed run bakes the same seeds into its own graph and replays it."""
    a, b1, b = _stop_and_resume(tmp_path, 12, 5, graph=True, precision="bf16")
    assert a["replays"] == 12 and b["replays"] == 7
    assert torch.equal(a["flat"], b1["flat"])                    # (writing checkpoints does not disturb a graphed run)
    g = torch.load(W.ckpt_at(tmp_path, "b", 5), map_location="cpu")["trainer_state"]["graph"]
    assert g["counter"] == 5 and g["rng"].get("dropout_seed_counter", 0) == 0 and "cpu" not in g["rng"]["train_generators"]


def test_resume_refuses_an_eager_continuation_of_a_graphed_run(tmp_path):
    kw = dict(device="cuda", model_kw=dict(backend="hip", precision="bf16"))
    W.run_fit(tmp_path, "g", 8, 4, graph=True, **kw)
    with pytest.raises(ValueError, match="graph-captured training step"):
        W.run_fit(tmp_path, "g", 8, 0, ckpt_path=W.ckpt_at(tmp_path, "g", 4), graph=False, **kw)


def test_resume_is_bitwise_the_uninterrupted_run_file_backed_module(tmp_path):
    """The file-backed module with its real HIP launch per batch (5 batches per epoch: K = 3 mid-epoch, N = 8 in the next epoch),
    one validation pass before K and three after."""
    files = W.write_files(tmp_path / "camels")
    kw = dict(device="cuda", val=2, model_kw=dict(backend="hip", precision="bf16"), dm=lambda: W.make_astro(files, cpu=False))
    a = W.run_fit(tmp_path, "a", 8, 0, **kw)
    W.run_fit(tmp_path, "b", 3, 3, **kw)
    b = W.run_fit(tmp_path, "b", 8, 0, ckpt_path=W.ckpt_at(tmp_path, "b", 3), **kw)
    W.assert_same_run(a, b, 3, 8)
    assert W.losses(b["history"], 3, "val_loss").numel() == 3


def test_graphed_step_puts_a_used_optimizer_state_back_after_its_warmup():
    """GraphedTrainStep built on an optimizer that has taken 3 eager steps: moments, step count and parameters after construction are
    bitwise those of before (they were zeroed: a resumed or loaded optimizer state was silently reset); the first replay is step 4."""
    from vdm4cdm_amd.trainer import GraphedTrainStep, clip_grad_norm_flat_
    W.fresh_process()
    vdm = W.make_model(backend="hip", precision="bf16").to(DEV).train()
    params = [p for p in vdm.parameters() if p.requires_grad]
    opt = vdm.configure_optimizers(capturable=True)
    batch = next(iter(W.make_synthetic().train_dataloader()))
    batch = {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in batch.items()}
    for i in range(3):
        loss = vdm.training_step(batch, i)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        clip_grad_norm_flat_(params, 0.5, True, want_norm=False)
        opt.step()
        del loss
    before = {k: v.detach().clone() for k, v in opt.state[params[0]].items()}
    flat = params[0].detach().clone()
    assert float(before["step"]) == 3 and before["exp_avg"].abs().max().item() > 0 and before["exp_avg_sq"].abs().max().item() > 0
    gs = GraphedTrainStep(vdm, opt, params, 0.5, batch)
    after = opt.state[params[0]]
    assert sorted(after) == sorted(before)
    for k in before:
        assert torch.equal(after[k], before[k]), f"{k} was not put back after the warm-up"
    assert torch.equal(params[0].detach(), flat) and gs.counter.item() == 0
    gs(batch)
    torch.cuda.synchronize()
    assert float(after["step"]) == 4 and gs.state_dict()["counter"] == 1 and not torch.equal(params[0].detach(), flat)
