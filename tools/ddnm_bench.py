"""ms per network evaluation of the DDNM sampler on the HIP backend, three ways, next to the ancestral graph step on the same box:

  eager    utils.get_ddnm_result without a new keyword (the reference-order Python loop, eager evaluations)
  generic  the graph path with generic callables (x0 kernel, AT(A(.)) as torch ops inside the captured step, update kernel)
  builtin  the graph path with a built-in operator (one fused kernel)

128^3, bf16 storage, chs 32..256, n = 250, l = 10 (2695 evaluations), B = 1 and B = 4, mask inpainting (half cube) and, for the
built-in path, 2x2x2 block means; the three runs alternate `--rounds` times.  Times are wall-clock around the whole call (tables, warm-up
and capture included) divided by the number of evaluations.  --kernels adds the fused kernels alone (with and without the x_r
write) against their HBM floors.  One process; every run has a deadline of its own (the process exits with status 124 when a run
overstays it) and the first failure ends the tool.  The deadline is a timer thread inside the process: it ends a run that hangs in
Python, not one stuck inside the driver, so run the tool itself under `timeout` with a kill escalation as well.  Prints one JSON line
per run.

    timeout -k 10 1100 python tools/ddnm_bench.py [--n 250] [--l 10] [--batches 1,4] [--rounds 3] [--deadline 300] [--kernels]
"""
import argparse
import json
import os
import sys
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def deadline(seconds, what):
    def fire():
        print(json.dumps({"run": what, "error": f"deadline of {seconds} s passed"}), flush=True)
        os._exit(124)
    t = threading.Timer(seconds, fire)
    t.daemon = True
    t.start()
    return t


def timed(fn, seconds, what):
    t = deadline(seconds, what)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        t.cancel()
    assert torch.isfinite(out).all(), f"{what}: non-finite result"
    return dt


def make_vdm(D):
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.vdm_model import LightVDM
    net = CUNet(shape=(1, D, D, D), chs=[32, 64, 128, 256], s_conditioning_channels=1, v_conditioning_dims=[6], t_conditioning=True,
                norm_groups=8, mid_attn=False, dropout_prob=0.1, conv_padding_mode="zeros", n_attention_heads=4, backend="hip",
                precision="bf16")
    net.reset_parameters(generator=torch.Generator().manual_seed(42), zero_init_std=0.02)
    return LightVDM(score_model=net, draw_figure=None, gamma_min=-13.3, gamma_max=13.3).to(DEV).eval()


def kernel_bench(D, B, reps=200):
    """The fused kernels alone at [B, 1, D, D, D]: us per launch with and without the x_r write, against 4 reads + 2 writes (mask) and
    2 reads + 2 writes (block mean) of the cube at the measured time."""
    from vdm4cdm_amd import hip_ops as ops
    shape = (B, 1, D, D, D)
    g = torch.Generator().manual_seed(0)
    z, eh, y = (torch.randn(shape, generator=g).to(DEV) for _ in range(3))
    m = (torch.rand(shape, generator=g) < 0.5).float().to(DEV)
    yb = torch.randn((B, 1, D // 2, D // 2, D // 2), generator=g).to(DEV)
    yx = torch.randn((B, 1, D, D, D // 2), generator=g).to(DEV)
    y8 = torch.randn((B, 1, D // 8, D // 8, D // 8), generator=g).to(DEV)
    xr = torch.empty_like(z)
    coef = torch.tensor([[1.0, 0.5, 0.9, 0.1, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float32, device=DEV)
    sched = torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    t = ops.DdnmTables(coef, sched, torch.arange(B, dtype=torch.int64, device=DEV))
    cube = z.numel() * 4
    runs = {"mask": (lambda o: ops.ddnm_mask_step(z, eh, m, y, t, None, o), 4),
            "blockmean_2x2x2": (lambda o: ops.ddnm_blockmean_step(z, eh, yb, (2, 2, 2), t, None, o), 2),
            "blockmean_1x1x2": (lambda o: ops.ddnm_blockmean_step(z, eh, yx, (1, 1, 2), t, None, o), 2),
            "blockmean_8x8x8": (lambda o: ops.ddnm_blockmean_step(z, eh, y8, (8, 8, 8), t, None, o), 2)}
    for name, (fn, reads) in runs.items():
        for o in (xr, None):
            for _ in range(10):
                fn(o)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn(o)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / reps
            moved = cube * (reads + (2 if o is not None else 1))
            print(json.dumps({"run": f"kernel:{name}", "B": B, "x_r_written": o is not None, "us": round(us, 2),
                              "TB_per_s": round(moved / us * 1e-6, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=250)
    ap.add_argument("--l", type=int, default=10)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--deadline", type=int, default=300, help="seconds allowed to one run")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    from vdm4cdm_amd import utils
    from vdm4cdm_amd.vdm_model import ddnm_schedule
    D = a.size
    vdm = make_vdm(D)
    E = len(ddnm_schedule(a.n, a.l)["k"])
    g = torch.Generator().manual_seed(1)
    for B in [int(b) for b in a.batches.split(",")]:
        shape = (B, 1, D, D, D)
        s = torch.randn(shape, generator=g).to(DEV)
        v = [torch.rand(B, 6, generator=g).to(DEV)]
        x = torch.randn(shape, generator=g).to(DEV)
        mask = torch.zeros((1, 1, D, D, D), device=DEV)
        mask[..., : D // 2] = 1.0
        op_m, op_b = utils.MaskOperator(mask), utils.BlockMeanOperator((2, 2, 2))
        y_m, y_b = op_m.A(x), op_b.A(x)
        kw = dict(n_sampling_steps=a.n, l=a.l, s_conditioning=s, v_conditionings=v)
        A = AT = lambda t: t * mask
        runs = {
            "eager": lambda: utils.get_ddnm_result(vdm, y_m, A, AT, **kw),
            "generic": lambda: utils.get_ddnm_result(vdm, y_m, A, AT, seeds=list(range(B)), **kw),
            "builtin": lambda: utils.get_ddnm_result(vdm, y_m, seeds=list(range(B)), operator=op_m, **kw),
            "builtin_blockmean": lambda: utils.get_ddnm_result(vdm, y_b, seeds=list(range(B)), operator=op_b, **kw),
        }
        dt = timed(lambda: vdm.draw_samples(batch_size=B, n_sampling_steps=a.n, seeds=list(range(B)), s_conditioning=s, v_conditionings=v),
                   a.deadline, "ancestral warm-up")
        for r in range(a.rounds):
            dt = timed(lambda: vdm.draw_samples(batch_size=B, n_sampling_steps=a.n, seeds=list(range(B)), s_conditioning=s, v_conditionings=v),
                       a.deadline, "ancestral")
            print(json.dumps({"run": "ancestral", "B": B, "round": r, "ms_per_eval": round(dt * 1e3 / a.n, 4), "evals": a.n}), flush=True)
            for name, fn in runs.items():
                dt = timed(fn, a.deadline, name)
                print(json.dumps({"run": name, "B": B, "round": r, "ms_per_eval": round(dt * 1e3 / E, 4), "evals": E, "seconds": round(dt, 2)}),
                      flush=True)
        if a.kernels:
            kernel_bench(D, B)


if __name__ == "__main__":
    main()
