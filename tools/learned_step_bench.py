"""ms per training step, fixed-linear vs learned-linear noise schedule, on the HIP backend (eager steps: training_step + backward +
clip + AdamW, as Trainer runs a learned step).  Configs: C3 (128^3, batch 2, chs 32..256, bf16) and train3D (128^3, batch 2,
chs 48..384, bf16).  Prints one JSON line per (config, schedule).

    python tools/learned_step_bench.py [--steps 20] [--warmup 3] [--configs c3,train3d]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"c3": (128, 2, [32, 64, 128, 256]), "train3d": (128, 2, [48, 96, 192, 384])}


def run(cfg, schedule, steps, warmup):
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.trainer import clip_grad_norm_flat_
    from vdm4cdm_amd.vdm_model import LightVDM
    D, B, chs = CONFIGS[cfg]
    dev = "cuda:0"
    torch.manual_seed(42)
    net = CUNet(shape=(1, D, D, D), chs=chs, s_conditioning_channels=1, v_conditioning_dims=[6], t_conditioning=True, norm_groups=8,
                mid_attn=False, dropout_prob=0.1, conv_padding_mode="zeros", n_attention_heads=4, backend="hip", precision="bf16")
    net.reset_parameters(generator=torch.Generator().manual_seed(42), zero_init_std=0.02)
    vdm = LightVDM(score_model=net, draw_figure=None, gamma_min=-13.3, gamma_max=13.3, noise_schedule=schedule).to(dev).train()
    opt = vdm.configure_optimizers()
    params = [p for p in vdm.parameters() if p.requires_grad]
    b = SyntheticAstroDataModule(cropsize=D, batch_size=B, seed=1000)._make_batch(1000, B)
    batch = {"x": b["x"].to(dev), "conditioning": b["conditioning"].to(dev), "conditioning_values": [b["conditioning_values"][0].to(dev)]}

    def step():
        loss = vdm.training_step(batch, 0)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        clip_grad_norm_flat_(params, 0.5, use_hip=True, want_norm=False)
        opt.step()
        return loss

    for _ in range(2 + warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return {"config": cfg, "schedule": schedule, "ms_per_step": round(ms, 3), "steps": steps, "loss": float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="c3,train3d")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "learned_step_bench needs a GPU"
    for cfg in args.configs.split(","):
        for schedule in ("fixed_linear", "learned_linear", "fixed_linear", "learned_linear"):      # alternating: two of each
            print(json.dumps(run(cfg, schedule, args.steps, args.warmup)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
