"""What the exponential moving average of the weights (LightVDM(ema_decay=)) costs on the HIP backend: ms per training step of the C3
configuration (128^3, batch 2, chs 32..256, bf16, dropout 0.1) with EMA off and on, for the eager step of bench.py (training_step +
backward + clip + AdamW) and for the graph-captured step (trainer.GraphedTrainStep, `graph_step`).

Both models live in ONE process and are timed in alternating rounds (off, on, off, on, ...), `--steps` steps per round behind a device
synchronise (0.6 s per window at the defaults), so that clock drift and other tenants of the host hit both alike.  Reported per leg and
setting: the median over the rounds and the spread (min, max of ALL rounds: an outlier stays in it) - a difference between the two below
the spread of either is not a difference.  The eager `off` row is the workload of `python bench.py --gpus 1`.  EMA adds one
vdm_ema_update launch over the flat parameter vector (12 bytes per parameter: two reads, one write) and one vdm_step_inc per step.

    python tools/ema_bench.py [--rounds 5] [--steps 50] [--warmup 5] [--cube 128] [--decay 0.9999]

Prints one JSON line per (leg, ema).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHS, B = [32, 64, 128, 256], 2


def build(decay, D, dev):
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.vdm_model import LightVDM
    torch.manual_seed(42)
    net = CUNet(shape=(1, D, D, D), chs=CHS, s_conditioning_channels=1, v_conditioning_dims=[6], t_conditioning=True, norm_groups=8,
                mid_attn=False, dropout_prob=0.1, conv_padding_mode="zeros", n_attention_heads=4, backend="hip", precision="bf16")
    net.reset_parameters(generator=torch.Generator().manual_seed(42), zero_init_std=0.02)
    vdm = LightVDM(score_model=net, draw_figure=None, gamma_max=13.3, learning_rate=3.0e-4, ema_decay=decay).to(dev).train()
    b = SyntheticAstroDataModule(cropsize=D, batch_size=B, seed=1000)._make_batch(1000, B)
    batch = {"x": b["x"].to(dev), "conditioning": b["conditioning"].to(dev), "conditioning_values": [b["conditioning_values"][0].to(dev)]}
    return vdm, batch


def eager_stepper(vdm, batch):
    from vdm4cdm_amd.trainer import clip_grad_norm_flat_
    opt = vdm.configure_optimizers()
    params = [p for p in vdm.parameters() if p.requires_grad]

    def step():
        loss = vdm.training_step(batch, 0)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        clip_grad_norm_flat_(params, 0.5, use_hip=True, want_norm=False)
        opt.step()
        return loss
    return step


def graph_stepper(vdm, batch):
    from vdm4cdm_amd.trainer import GraphedTrainStep
    gs = GraphedTrainStep(vdm, vdm.configure_optimizers(capturable=True), [p for p in vdm.parameters() if p.requires_grad], 0.5, batch)
    return lambda: gs(batch)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, out


def report(leg, ema, ms, **extra):
    print(json.dumps(dict(leg=leg, ema=ema, ms_per_step_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3),
                          ms_max=round(max(ms), 3), rounds=[round(m, 3) for m in ms], **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cube", type=int, default=128)
    ap.add_argument("--decay", type=float, default=0.9999)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ema_bench needs a GPU"
    dev, D = "cuda:0", args.cube
    for leg, make in (("eager", eager_stepper), ("graph_step", graph_stepper)):
        models = {name: build(decay, D, dev) for name, decay in (("off", None), ("on", args.decay))}
        steppers = {}
        for name, (vdm, batch) in models.items():        # (a graphed step is built on a model that has taken no eager step)
            steppers[name] = make(vdm, batch)
            for _ in range(2 + args.warmup):
                steppers[name]()
        ms, loss = {name: [] for name in models}, {}
        for _ in range(args.rounds):
            for name in models:
                t, l = timed(steppers[name], args.steps)
                ms[name].append(t)
                loss[name] = float(l.detach())
        for name, (vdm, _) in models.items():
            n_par = sum(p.numel() for p in vdm.parameters())
            report(leg, name, ms[name], steps_per_round=args.steps, cube=D, batch=B, parameters=n_par, loss=loss[name],
                   ema_updates=None if vdm.ema is None else vdm.ema.num_updates)
        del steppers, models
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
