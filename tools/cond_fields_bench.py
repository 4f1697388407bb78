"""What K conditioning fields cost on the HIP backend: ms per training step of the C3 configuration (128^3, batch 2, chs 32..256, bf16,
dropout 0.1; the eager step of bench.py: training_step + backward + clip + AdamW) for K = 1, 2, 3, and ms per captured sampling step
(128^3, batch 1, the hipGraph replay of draw_samples) for K = 1 and 3.

All models live in ONE process and are timed in alternating rounds (K = 1, 2, 3, 1, 2, 3, ...), `--steps` steps per round behind a
device synchronise (0.6 s per window at the defaults), so that clock drift and other tenants of the host hit every K alike.  Reported per
K: the median over the rounds and the spread (min, max of ALL rounds: an outlier stays in it) - a difference between two K below the
spread of either is not a difference.  The K = 1 row is the workload of
`python bench.py --gpus 1`: the two must agree within that spread.

    python tools/cond_fields_bench.py [--rounds 5] [--steps 50] [--warmup 5] [--sample-steps 250] [--cube 128]

Prints one JSON line per (leg, K).
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
NAMES = ["Mstar", "Mgas", "T"]


def build(K, D, dev):
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.vdm_model import LightVDM
    torch.manual_seed(42)
    net = CUNet(shape=(1, D, D, D), chs=CHS, s_conditioning_channels=K, v_conditioning_dims=[6], t_conditioning=True, norm_groups=8,
                mid_attn=False, dropout_prob=0.1, conv_padding_mode="zeros", n_attention_heads=4, backend="hip", precision="bf16")
    net.reset_parameters(generator=torch.Generator().manual_seed(42), zero_init_std=0.02)
    vdm = LightVDM(score_model=net, draw_figure=None, gamma_max=13.3, learning_rate=3.0e-4).to(dev)
    b = SyntheticAstroDataModule(cropsize=D, batch_size=B, seed=1000, channel_names=NAMES[:K] + ["Mcdm"])._make_batch(1000, B)
    batch = {"x": b["x"].to(dev), "conditioning": b["conditioning"].to(dev), "conditioning_values": [b["conditioning_values"][0].to(dev)]}
    assert batch["conditioning"].shape[1] == K
    return vdm, batch


def train_stepper(vdm, batch):
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


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, out


def report(leg, K, ms, **extra):
    print(json.dumps(dict(leg=leg, K=K, ms_per_step_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                          rounds=[round(m, 3) for m in ms], **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sample-steps", type=int, default=250)
    ap.add_argument("--cube", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cond_fields_bench needs a GPU"
    dev, D = "cuda:0", args.cube
    # ---- training step: K = 1, 2, 3 alternating
    models = {K: build(K, D, dev) for K in (1, 2, 3)}
    steppers = {}
    for K, (vdm, batch) in models.items():
        vdm.train()
        steppers[K] = train_stepper(vdm, batch)
        for _ in range(2 + args.warmup):
            steppers[K]()
    ms, loss = {K: [] for K in models}, {}
    for _ in range(args.rounds):
        for K in models:
            t, l = timed(steppers[K], args.steps)
            ms[K].append(t)
            loss[K] = float(l.detach())
    for K in models:
        report("train_step", K, ms[K], steps_per_round=args.steps, cube=D, batch=B, loss=loss[K])
    # ---- sampling step: K = 1 and 3 alternating (one chain of --sample-steps captured steps per round; the capture is inside the window,
    # so the per-step figure carries 1 / sample_steps of it - the same for both K)
    del steppers
    for K in (1, 3):
        models[K][0].eval()
        for p in models[K][0].parameters():
            p.grad = None
    torch.cuda.empty_cache()
    sms = {1: [], 3: []}

    def chain(K):
        vdm, batch = models[K]
        return vdm.draw_samples(batch_size=1, n_sampling_steps=args.sample_steps, seed=1234, s_conditioning=batch["conditioning"][:1],
                                v_conditionings=[batch["conditioning_values"][0][:1]])
    for K in sms:
        chain(K)                                             # warm-up: packs the forward weights, sizes the allocator
    for _ in range(args.rounds):
        for K in sms:
            t, z = timed(lambda: chain(K), 1)
            sms[K].append(t / args.sample_steps)
            assert torch.isfinite(z).all()
    for K in sms:
        report("sampling_step", K, sms[K], steps_per_chain=args.sample_steps, cube=D, batch=1)


if __name__ == "__main__":
    main()
