#!/usr/bin/env python
"""Time of vdm_log_moments on one slab (default 2^28 floats = 1 GiB of "cdm"-like values), next to the expression a user would
otherwise write on the same slab - v = torch.log10(x.double() + alpha); v.mean(); v.std(unbiased=False) - which needs two float64
temporaries of twice the slab.  Device events, `--warmup` untimed and `--iters` timed launches each; one JSON line.
    python tools/log_moments_bench.py [--log2n 28] [--warmup 5] [--iters 20]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vdm4cdm_amd import _lib, data, hip_ops as ops  # noqa: E402


def timed(fn, warmup, iters):
    """(mean, min) ms per call: one event pair per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return sum(ms) / len(ms), min(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev, n, alpha, pivot = "cuda:0", 1 << a.log2n, 1.0, 10.0
    x = torch.empty(n, device=dev)
    for i in range(0, n, 1 << 24):                             # (filled in pieces: no float64 temporary of the whole slab)
        g = torch.Generator(device=dev).manual_seed(i)
        x[i:i + (1 << 24)] = 10.0 ** (torch.randn(min(1 << 24, n - i), device=dev, generator=g) * 0.55 + 10.02)
    buf = torch.empty(ops.LOG_MOMENTS_OUT + ops.LOG_MOMENTS_WS, dtype=torch.float64, device=dev)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def kernel():
        _lib.check(L.vdm_log_moments(x.data_ptr(), n, alpha, pivot, buf.data_ptr(), buf[ops.LOG_MOMENTS_OUT:].data_ptr(), stream))

    def eager():
        v = torch.log10(x.double() + alpha)
        return v.mean(), v.std(unbiased=False)

    k_mean, k_min = timed(kernel, a.warmup, a.iters)
    r = buf[:ops.LOG_MOMENTS_OUT].tolist()
    _, mean, std, _, _, _ = data.merge_log_moments([dict(zip(("n_valid", "S1", "S2", "min", "max", "n_bad"), r))], pivot)
    e_mean, e_min = timed(eager, a.warmup, a.iters)
    m, s = eager()
    print(json.dumps({"n": n, "kernel_ms": round(k_mean, 4), "kernel_ms_min": round(k_min, 4), "eager_ms": round(e_mean, 4),
                      "eager_ms_min": round(e_min, 4), "ratio": round(e_mean / k_mean, 2), "kernel_gelem_s": round(n / k_mean / 1e6, 1),
                      "kernel_tb_s": round(4 * n / k_mean / 1e9, 3), "mean": mean, "std": std, "mean_minus_eager": mean - m.item(),
                      "std_minus_eager": std - s.item(), "n_bad": int(r[5]), "finite": math.isfinite(mean)}))


if __name__ == "__main__":
    main()
