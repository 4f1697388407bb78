"""ms per flow-matching (SFM) training step on the HIP backend, three ways: the unfused eager step (the chain diffuse -> diffuse ->
pack_input -> VDM loss kernel, VDM4CDM_EXPERIMENT=fused_head=0), the fused eager step (vdm_sfm_head + vdm_sfm_loss) and the fused step
captured in a hipGraph (trainer.GraphedTrainStep) - at 32^3, 64^3 and 128^3 with bf16 storage, chs 32..256, batch 2, dropout 0.1.  A step
is training_step + backward + clip + AdamW, as Trainer runs it.

The three configurations of a cube live in ONE process, each with its own model and optimizer, and are timed in alternating windows
(unfused, fused, graphed, unfused, ...), every window behind a device synchronise, so that clock drift and other tenants of the host hit all
three alike.  Reported per configuration: the median over the windows and the spread (min, max of ALL windows) - a difference between two
configurations below the spread of either is not a difference.

    python tools/sfm_step_bench.py [--rounds 5] [--cubes 32,64,128] [--warmup 5] [--sigma 0.0]

Prints one JSON line per (cube, configuration).
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
STEPS = {32: 100, 64: 50, 128: 30}                              # steps per window (0.2 - 0.4 s)
MODES = ("unfused_eager", "fused_eager", "graphed")


def build(D, dev, sigma):
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.sfm_model import LightSFM
    torch.manual_seed(42)
    net = CUNet(shape=(1, D, D, D), chs=CHS, s_conditioning_channels=1, v_conditioning_dims=[6], t_conditioning=True, norm_groups=8,
                mid_attn=False, dropout_prob=0.1, conv_padding_mode="zeros", n_attention_heads=4, backend="hip", precision="bf16")
    net.reset_parameters(generator=torch.Generator().manual_seed(42), zero_init_std=0.02)
    sfm = LightSFM(velocity_model=net, draw_figure=None, learning_rate=3.0e-4, sigma=sigma).to(dev).train()
    b = SyntheticAstroDataModule(cropsize=D, batch_size=B, seed=1000)._make_batch(1000, B)
    batch = {"x0": b["conditioning"].to(dev), "x1": b["x"].to(dev), "conditioning_values": [b["conditioning_values"][0].to(dev)]}
    return sfm, batch


def stepper(mode, D, dev, sigma):
    import vdm4cdm_amd.sfm_model as sm
    from vdm4cdm_amd.trainer import GraphedTrainStep, clip_grad_norm_flat_
    sfm, batch = build(D, dev, sigma)
    params = [p for p in sfm.parameters() if p.requires_grad]
    if mode == "graphed":
        sm.FUSED_HEAD = True
        gs = GraphedTrainStep(sfm, sfm.configure_optimizers(capturable=True), params, 0.5, batch)
        return lambda: gs(batch)
    opt = sfm.configure_optimizers()

    def step():
        sm.FUSED_HEAD = mode == "fused_eager"
        loss = sfm.training_step(batch, 0)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        clip_grad_norm_flat_(params, 0.5, use_hip=True, want_norm=False)
        opt.step()
        return loss
    return step


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cubes", default="32,64,128")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sfm_step_bench needs a GPU"
    dev = "cuda:0"
    for D in (int(c) for c in args.cubes.split(",")):
        steps = STEPS.get(D, 30)
        steppers = {m: stepper(m, D, dev, args.sigma) for m in MODES}
        for m in MODES:
            for _ in range(2 + args.warmup):
                steppers[m]()
        ms, loss = {m: [] for m in MODES}, {}
        for _ in range(args.rounds):
            for m in MODES:
                t, l = timed(steppers[m], steps)
                ms[m].append(t)
                loss[m] = float(l.detach())
        for m in MODES:
            print(json.dumps(dict(cube=D, mode=m, ms_per_step_median=round(statistics.median(ms[m]), 3), ms_min=round(min(ms[m]), 3),
                                  ms_max=round(max(ms[m]), 3), windows=[round(v, 3) for v in ms[m]], steps_per_window=steps, batch=B,
                                  sigma=args.sigma, loss=loss[m])), flush=True)
        del steppers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
