"""What a sampling step costs under the stochastic ancestral sampler and under the second-order multistep solver (sampler="dpm2m"): ms
per captured step at 128^3, batch 1 (chs 32..256, bf16: the network of bench.py's sampling half; the hipGraph replay of draw_samples).

Both samplers run on ONE model in ONE process, timed in alternating windows (ancestral, dpm2m, ancestral, dpm2m, ...), one chain of
`--sample-steps` steps per window behind a device synchronise, so that clock drift and other tenants of the host hit both alike.  The
capture is inside the window: the per-step figure carries 1 / sample_steps of it, the same for both.  Reported per sampler: the median
over the windows and the spread (min, max of ALL windows: an outlier stays in it) - a difference below the spread of either is not a
difference.  The yardstick is the ancestral step measured here, in the same process.

This measures steps per second only.  It says nothing about how many steps a sampler needs: no trained weights ship with the
repository, and sample quality is not measured.

    python tools/sampler_order_bench.py [--rounds 5] [--sample-steps 250] [--cube 128]

Prints one JSON line per sampler.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHS = [32, 64, 128, 256]
SAMPLERS = ("ancestral", "dpm2m")


def build(D, dev):
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.vdm_model import LightVDM
    net = CUNet(shape=(1, D, D, D), chs=CHS, s_conditioning_channels=1, v_conditioning_dims=[6], t_conditioning=True, norm_groups=8,
                mid_attn=False, dropout_prob=0.1, conv_padding_mode="zeros", n_attention_heads=4, backend="hip", precision="bf16")
    net.reset_parameters(generator=torch.Generator().manual_seed(42), zero_init_std=0.02)
    vdm = LightVDM(score_model=net, draw_figure=None, gamma_max=13.3, learning_rate=3.0e-4).to(dev).eval()
    b = SyntheticAstroDataModule(cropsize=D, batch_size=1, seed=1000, channel_names=["Mstar", "Mcdm"])._make_batch(1000, 1)
    return vdm, b["conditioning"].to(dev), [b["conditioning_values"][0].to(dev)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample-steps", type=int, default=250)
    ap.add_argument("--cube", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sampler_order_bench needs a GPU"
    dev, D, n = "cuda:0", args.cube, args.sample_steps
    vdm, s, v = build(D, dev)

    def chain(name):
        return vdm.draw_samples(batch_size=1, n_sampling_steps=n, seed=1234, sampler=name, s_conditioning=s, v_conditionings=v)
    for name in SAMPLERS:
        chain(name)                                          # warm-up: packs the forward weights, sizes the allocator
    ms = {name: [] for name in SAMPLERS}
    for _ in range(args.rounds):
        for name in SAMPLERS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            z = chain(name)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / n)
            assert torch.isfinite(z).all()
    for name in SAMPLERS:
        m = ms[name]
        print(json.dumps(dict(leg="sampling_step", sampler=name, ms_per_step_median=round(statistics.median(m), 4), ms_min=round(min(m), 4),
                              ms_max=round(max(m), 4), steps_per_s=round(1e3 / statistics.median(m), 1), windows=[round(x, 4) for x in m],
                              steps_per_chain=n, cube=D, batch=1)), flush=True)


if __name__ == "__main__":
    main()
