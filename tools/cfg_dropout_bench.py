"""What conditioning dropout (classifier-free guidance training, VDM(p_uncond=, cfg_drop=)) costs on the HIP backend: ms per training
step of the C3 configuration (128^3, batch 2, chs 32..256, bf16, dropout 0.1) with p_uncond = 0 and p_uncond = 0.1, for the eager step
of bench.py (training_step + backward + clip + AdamW) and for the graph-captured step (trainer.GraphedTrainStep, `graph_step`).

Both models live in ONE process and are timed in alternating rounds (p = 0, 0.1, 0, 0.1, ...), `--steps` steps per round behind a
device synchronise (0.6 s per window at the defaults), so that clock drift and other tenants of the host hit both alike.  Reported per
p: the median over the rounds and the spread (min, max of ALL rounds: an outlier stays in it) - a difference between the two below the
spread of either is not a difference.  The eager p = 0 row is the workload of `python bench.py --gpus 1`.  p = 0.1 adds one
vdm_cond_keep launch, one vdm_mask_rows launch per vector conditioning and direction, and the keep-aware head; dropped rows skip the
read of their conditioning planes.

    python tools/cfg_dropout_bench.py [--rounds 5] [--steps 50] [--warmup 5] [--cube 128] [--cfg-drop vs] [--p 0.1]

Prints one JSON line per (leg, p_uncond).
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


def build(p, drop, D, dev):
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.vdm_model import LightVDM
    torch.manual_seed(42)
    net = CUNet(shape=(1, D, D, D), chs=CHS, s_conditioning_channels=1, v_conditioning_dims=[6], t_conditioning=True, norm_groups=8,
                mid_attn=False, dropout_prob=0.1, conv_padding_mode="zeros", n_attention_heads=4, backend="hip", precision="bf16")
    net.reset_parameters(generator=torch.Generator().manual_seed(42), zero_init_std=0.02)
    vdm = LightVDM(score_model=net, draw_figure=None, gamma_max=13.3, learning_rate=3.0e-4, p_uncond=p, cfg_drop=drop).to(dev).train()
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


def report(leg, p, ms, **extra):
    print(json.dumps(dict(leg=leg, p_uncond=p, ms_per_step_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3),
                          ms_max=round(max(ms), 3), rounds=[round(m, 3) for m in ms], **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cube", type=int, default=128)
    ap.add_argument("--cfg-drop", default="vs", choices=["v", "s", "vs"])
    ap.add_argument("--p", type=float, default=0.1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cfg_dropout_bench needs a GPU"
    dev, D = "cuda:0", args.cube
    for leg, make in (("eager", eager_stepper), ("graph_step", graph_stepper)):
        models = {p: build(p, args.cfg_drop, D, dev) for p in (0.0, args.p)}
        steppers = {}
        for p, (vdm, batch) in models.items():           # (a graphed step is built on a model that has taken no eager step)
            steppers[p] = make(vdm, batch)
            for _ in range(2 + args.warmup):
                steppers[p]()
        ms, loss, kept = {p: [] for p in models}, {}, {}
        for _ in range(args.rounds):
            for p in models:
                t, l = timed(steppers[p], args.steps)
                ms[p].append(t)
                loss[p] = float(l.detach())
                k = models[p][0].model.last_cond_keep
                kept[p] = None if k is None else k.tolist()
        for p in models:
            report(leg, p, ms[p], steps_per_round=args.steps, cube=D, batch=B, cfg_drop=args.cfg_drop, loss=loss[p], last_cond_keep=kept[p])
        del steppers, models
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
