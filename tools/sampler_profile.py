#!/usr/bin/env python
"""Reverse-diffusion sampler alone (BASELINE config C5: 128^3, hipGraph-captured denoise step) - the program to put behind
rocprofv3 --kernel-trace --stats for the per-kernel anatomy of one sampling step, and the per-chain cost of batched sampling
(--batch B: B chains per replay, each keyed by its own seed as generate_3D samples them with VDM4CDM_SAMPLE_BATCH=B).
    python tools/sampler_profile.py [--steps 100] [--cube 128] [--batch 1] [--chs 32,64,128,256] [--padding zeros|circular]
                                    [--precision bf16] [--repeats 3] [--one-seed]
--one-seed (batch 1): time the one-seed update (seed=, ancestral_kernel) as well as the row-keyed one (seeds=[s]) in the same process.
Prints one JSON line: ms per step, ms per step per chain (per repeat), torch.cuda.max_memory_allocated of the timed draws."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def build_model(D, chs, precision, padding, device, seed=42):
    """bench.build_model with the padding mode chosen on the command line."""
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.vdm_model import LightVDM
    torch.manual_seed(seed)
    net = CUNet(shape=(1, D, D, D), chs=chs, s_conditioning_channels=1, v_conditioning_dims=[6], t_conditioning=True,
                norm_groups=8, mid_attn=False, dropout_prob=0.1, conv_padding_mode=padding, n_attention_heads=4,
                backend="hip", precision=precision)
    net.reset_parameters(generator=torch.Generator().manual_seed(seed), zero_init_std=0.02)
    return LightVDM(score_model=net, draw_figure=None, gamma_max=13.3, learning_rate=3.0e-4).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--cube", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--chs", type=str, default="32,64,128,256")
    ap.add_argument("--padding", choices=["zeros", "circular"], default="zeros")
    ap.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--one-seed", action="store_true")
    args = ap.parse_args()
    from vdm4cdm_amd.entry import chain_seed
    dev = "cuda:0"
    chs = [int(c) for c in args.chs.split(",")]
    vdm = build_model(args.cube, chs, args.precision, args.padding, dev).eval()
    b = bench.make_batch(args.cube, 1, 0, dev)                          # one conditioning cube for all chains (as generate_3D)
    kw = dict(s_conditioning=b["conditioning"], v_conditionings=b["conditioning_values"])
    seeds = [chain_seed(c) for c in range(args.batch)]

    def timed(**extra):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vdm.draw_samples(batch_size=args.batch, n_sampling_steps=args.steps, **kw, **extra)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    vdm.draw_samples(batch_size=args.batch, n_sampling_steps=3, seeds=seeds, **kw)          # packs the weights, warms the allocator
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    ms = [timed(seeds=seeds) for _ in range(args.repeats)]
    out = {"cube": args.cube, "chs": chs, "padding": args.padding, "precision": args.precision, "steps": args.steps, "batch": args.batch,
           "ms_per_step": ms, "ms_per_step_per_chain": [m / args.batch for m in ms],
           "max_memory_allocated_GiB": torch.cuda.max_memory_allocated(dev) / 2 ** 30}
    if args.one_seed:
        assert args.batch == 1, "--one-seed compares the two updates at batch 1"
        out["ms_per_step_one_seed"] = [timed(seed=seeds[0]) for _ in range(args.repeats)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
