"""Reference of the exponential moving average of the weights (vdm_ema_update / ema.EmaWeights), and the small training runs the EMA
tests share.

The recurrence, for update number k (k = 0 for the first one):

    q  = (1 + k) / (10 + k)                 d = min(decay, q) under warm-up, else decay
    w  = 1 - d
    e' = e + w * (p - e)

`ema_step` evaluates it in numpy float32 in exactly this order.  numpy rounds every float32 operation on its own (IEEE round to nearest
even), which is what the kernel and the torch path are required to do, so the comparison needs no tolerance.

`ema_step64` is the same recurrence in float64 with the SAME float32 weight w (w is a parameter of the per-element update; its own two
roundings are covered by the bit-for-bit comparison).  With u = 2^-24 the float32 result differs from it by three roundings:

    s  = rn(p - e)  = (p - e)(1 + d1)         subtract
    m  = rn(w * s)  = w s (1 + d2)            multiply
    e' = rn(e + m)  = (e + m)(1 + d3)         add          |d1|, |d2|, |d3| <= u, and |x - rn(x)| <= u |rn(x)| as well

    e' - E = w (p - e)(d1 + d2 + d1 d2) + (e + m) d3,    so    |e' - E| <= (2u + u^2) w |p - e| + u |e'|          (`bound`)

each rounding relative to the size of its own result.  Since E is a convex combination of e and p, w |p - e| <= 2 w M with M =
max(|e|, |p|), which gives, up to u^2,

    |e' - E| <= c(w) u max(|e|, |p|, |e'|),    c(w) = 4 w + 1                                                      (`bound_max`)

That is at most THREE roundings of the largest of |e|, |p|, |e'| whenever w <= 1/2 (every update past the warm-up with decay >= 1/2),
and also for w = 1 (decay 0: the product is exact, d2 = 0, so c = 3).  For 1/2 < w < 1 - the first updates of the warm-up - three is NOT
a bound of correctly rounded arithmetic: at w = 0.9 (k = 0) the float32 recurrence above, evaluated by numpy, is up to 3.13 u max(...)
away from the float64 one (146 of the 2 097 159 elements of the largest test vector exceed 3), within c(0.9) = 4.6.  The kernel test
asserts both `bound` and `bound_max`.  The relative bound |d| <= u holds for normal results only: a product that falls into the
subnormal range is rounded to a multiple of 2^-149, an absolute error of at most 2^-150 (sums and differences of float32 values are
exact there), so both bounds carry that one term, TINY.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
TINY = 2.0 ** -150


def weight(decay, warmup, k):
    """w = 1 - d_k in float32: the integer sums first, each converted once, one division, one minimum, one subtraction."""
    d = np.float32(decay)
    if warmup:
        q = np.float32(1 + int(k)) / np.float32(10 + int(k))
        d = np.minimum(d, q)
    return np.float32(1.0) - d


def ema_step(e, p, decay, warmup, k):
    """One update of the float32 vector e towards p; returns the new vector (float32)."""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    w = weight(decay, warmup, k)
    with np.errstate(all="ignore"):
        return (e + w * (p - e)).astype(np.float32)          # float32 arrays and a float32 scalar: three float32 operations


def ema_step64(e, p, decay, warmup, k):
    w = np.float64(weight(decay, warmup, k))
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return e + w * (p - e)


def bound(e, p, e_new, decay, warmup, k):
    """(2u + u^2) w |p - e| + u |e'| per element, in float64 (module docstring)."""
    w = np.float64(weight(decay, warmup, k))
    e, p, e_new = (np.asarray(a, dtype=np.float64) for a in (e, p, e_new))
    return (2 * U + U * U) * w * np.abs(p - e) + U * np.abs(e_new) + TINY


def roundings(decay, warmup, k):
    """c(w) of the module docstring: 3 for w <= 1/2 and for w = 1, else 4 w + 1."""
    w = float(weight(decay, warmup, k))
    return 3.0 if (w <= 0.5 or w == 1.0) else 4.0 * w + 1.0


def bound_max(e, p, e_new, decay, warmup, k):
    """c(w) u max(|e|, |p|, |e'|) per element, in float64."""
    e, p, e_new = (np.abs(np.asarray(a, dtype=np.float64)) for a in (e, p, e_new))
    return roundings(decay, warmup, k) * U * (1 + U) * np.maximum(np.maximum(e, p), e_new) + TINY


def ema_sequence(params, decay, warmup, k0=0, shadow=None):
    """params: [p_0, p_1, ..., p_N] - the parameter vector before the first and after each of N steps.  Returns the shadows
    [s_0 = p_0 (or `shadow`), s_1, ..., s_N] where step i uses update number k0 + i - 1."""
    out = [np.asarray(params[0] if shadow is None else shadow, dtype=np.float32).copy()]
    for i, p in enumerate(params[1:]):
        out.append(ema_step(out[-1], p, decay, warmup, k0 + i))
    return out


# ---------------------------------------------------------------------------------------------- kernel-test inputs
SIZES = [1, 3, 4, 5, 1023, 4099, 2048 * 256 * 4 + 7]        # the last: one full sweep of the capped grid (2048 blocks x 256 x float4) + 7
ALIGNMENTS = ["aligned", "ema_off1", "p_off1"]
COUNTERS = [0, 1, 8, 9, 1000, None]                         # None: a NULL counter (k = 0)
DECAYS = [0.5, 0.999, 0.0]
PAD = 8                                                     # canary floats on each side of a vector
CANARY = 0x7FC12345                                         # a NaN payload: any arithmetic on it, or any write, changes the bits

_inputs = {}


def inputs(n):
    """(e, p) float32 of length n, computed once per n: normals with planted p == e, zeros, +-large, a denormal (where n allows)."""
    if n not in _inputs:
        rng = np.random.default_rng(1000 + n)
        e, p = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        planted = [(0.75, 0.75), (0.0, 0.0), (0.0, 1.5), (-2.0, 0.0), (1e30, -1e30), (-1e30, 3.0), (1e-40, 2e-40), (-0.0, 0.0)]
        for j, (a, b) in enumerate(planted):
            i = (j * 131 + 7) % n if n > len(planted) else None
            if i is not None:
                e[i], p[i] = a, b
        if n <= len(planted):                                # tiny vectors: the first planted pairs fill them
            for i in range(n):
                e[i], p[i] = planted[i % 3 if n > 1 else 0]
        e.setflags(write=False)
        p.setflags(write=False)
        _inputs[n] = (e, p)
    return _inputs[n]


# ---------------------------------------------------------------------------------------------- small training runs
def make_vdm(backend="torch", precision="fp32", schedule="fixed_linear", **kw):
    """The smallest network of the suite (tests/_resume_worker.py: 16^3, two levels, dropout on) under a LightVDM built with **kw."""
    import torch
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.vdm_model import LightVDM
    net = CUNet(shape=(1, 16, 16, 16), chs=[16, 32] if backend == "hip" else [8, 16], s_conditioning_channels=1, v_conditioning_dims=[6],
                t_conditioning=True, norm_groups=8, mid_attn=False, dropout_prob=0.1, conv_padding_mode="zeros", n_attention_heads=4,
                backend=backend, precision=precision)
    net.reset_parameters(generator=torch.Generator().manual_seed(21), zero_init_std=0.05)
    return LightVDM(score_model=net, draw_figure=None, gamma_min=-13.3, gamma_max=13.3, noise_schedule=schedule, learning_rate=3e-3, **kw)


def make_sfm(backend="torch", precision="fp32", **kw):
    import torch
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.sfm_model import LightSFM
    net = CUNet(shape=(1, 16, 16, 16), chs=[16, 32] if backend == "hip" else [8, 16], s_conditioning_channels=1, v_conditioning_dims=[6],
                t_conditioning=True, norm_groups=8, mid_attn=False, dropout_prob=0.1, conv_padding_mode="zeros", n_attention_heads=4,
                backend=backend, precision=precision)
    net.reset_parameters(generator=torch.Generator().manual_seed(21), zero_init_std=0.05)
    return LightSFM(velocity_model=net, draw_figure=None, learning_rate=3e-3, **kw)


def sfm_return_func(fields, params):
    return {"x0": fields[0], "x1": fields[1], "conditioning_values": [params]}


def make_dm(sfm=False):
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    kw = {"return_func": sfm_return_func} if sfm else {}
    return SyntheticAstroDataModule(cropsize=16, batch_size=2, n_train=8, n_val=4, seed=5, **kw)


def trainable(model):
    """The trainable tensors of a Light module, detached, in the order EmaWeights keeps its shadows: the network's flat vector first,
    then the module's own (gamma_b, gamma_w under the learned-linear schedule)."""
    flat = model.model.score_model.flat
    return [flat.detach()] + [p.detach() for p in model.parameters() if p.requires_grad and p is not flat]


def record_params(dm, model, log):
    """Makes `dm` append the model's trainable tensors (CPU numpy copies) to `log` every time the fit loop asks for a batch: entry i is
    the state after i real steps of this fit (the warm-up steps of a captured step happen between two requests and must leave no
    trace).  The caller appends the final state after fit."""
    orig = dm.train_dataloader

    def train_dataloader(rank=0, world=1, start_batch=0):
        it = orig(rank, world, start_batch=start_batch) if start_batch else orig(rank, world)
        for b in it:
            log.append(snapshot(model))
            yield b

    dm.train_dataloader = train_dataloader
    return dm


def snapshot(model):
    return [p.cpu().numpy().copy().reshape(-1) for p in trainable(model)]


def run_fit(root, name, make, steps, device="cpu", every=0, val=0, graph=False, ckpt_path=None, sfm=False):
    """One fit from a "fresh process" (tests/_resume_worker.fresh_process).  Returns {"model", "trainer", "params": per-step list of the
    trainable tensors (entry 0: before the first step of this fit), "shadows", "num_updates", "history"}."""
    import _resume_worker as W
    from vdm4cdm_amd.trainer import Trainer
    W.fresh_process()
    model, log = make(), []
    dm = record_params(make_dm(sfm), model, log)
    tr = Trainer(max_steps=steps, val_check_interval=val, gradient_clip_val=0.5, every_n_train_steps=every, default_root_dir=str(root),
                 experiment_name=name, device=device, enable_progress=False, log_every_n_steps=1, limit_val_batches=2, graph_step=graph)
    tr.fit(model, dm, **({} if ckpt_path is None else {"ckpt_path": ckpt_path}))
    log.append(snapshot(model))
    ema = model.ema
    return {"model": model, "trainer": tr, "params": log, "history": list(tr.history),
            "shadows": None if ema is None else [s.detach().cpu().numpy().copy().reshape(-1) for s in ema.shadows],
            "num_updates": None if ema is None else ema.num_updates}


def assert_shadows_follow_ref(run, decay, warmup, k0=0, start=None):
    """The run's final shadows are `ema_sequence` over its recorded per-step parameters, tensor by tensor, bit for bit."""
    n_steps = len(run["params"]) - 1
    assert run["num_updates"] == k0 + n_steps, f"counter {run['num_updates']} after {n_steps} real steps from {k0}"
    for t, got in enumerate(run["shadows"]):
        seq = [step[t] for step in run["params"]]
        want = ema_sequence(seq, decay, warmup, k0, None if start is None else start[t])[-1]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), \
            f"tensor {t}: {(got.view(np.int32) != want.view(np.int32)).sum()} of {got.size} shadow values differ from the float32 reference"
