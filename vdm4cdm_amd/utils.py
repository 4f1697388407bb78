"""Helpers the reference keeps in ``src/utils.py`` that sit on either side of the hot path.

* ``power`` / ``pk`` / ``get_ccs``: the acceptance metric (isotropic P(k), cross-correlation) -
  same estimator as /root/reference/src/utils.py:16-128, re-stated; runs on whatever device the field is on
  (rocFFT via ``torch.fft`` on the GPU).  Checked against golden vectors of the reference (tests/golden/pk_golden.npz).
* ``get_model`` / ``get_datamodule``: config -> model / data module with the reference's defaults
  (/root/reference/src/utils.py:401-475).
* ``get_ddnm_result``: the DDNM inpainting sampler (/root/reference/src/utils.py:277-304) on this package's VDM.
"""
import numpy as np
import torch

_SHELL_CACHE = {}


def _shells(size, device):
    """(kbin int64 [M], weights N int32 [M], |k| float32 [M]) for an rfftn grid of spatial `size`."""
    key = (tuple(size), str(device))
    hit = _SHELL_CACHE.get(key)
    if hit is not None:
        return hit
    rshape = tuple(size[:-1]) + (size[-1] // 2 + 1,)
    axes = []
    for ax, d in enumerate(rshape):
        j = torch.arange(d, dtype=torch.float32, device=device)
        if ax != len(rshape) - 1:
            j = torch.where(j > d // 2, j - d, j)            # signed frequencies on the full axes
        axes.append(j)
    grids = torch.meshgrid(*axes, indexing="ij")
    kmag = torch.sqrt(sum(g * g for g in grids)).flatten()
    w = torch.full(rshape, 2, dtype=torch.int32, device=device)  # Hermitian multiplicity of the half-spectrum
    w[..., 0] = 1
    if size[-1] % 2 == 0:
        w[..., -1] = 1
    out = (kmag.ceil().to(torch.int64), w.flatten(), kmag)
    _SHELL_CACHE[key] = out
    return out


def power(x, x2=None):
    """Shell-averaged (cross-)power of fields shaped (batch, channel, *spatial): mean over batch, sum over channels,
    integer-|k| shells by ceil, Hermitian-weighted, k=0 dropped, cut at the smallest Nyquist.  Returns (k, P, N)."""
    nd = x.dim() - 2
    size = tuple(x.shape[-nd:])
    kmax = min(size) // 2
    dims = tuple(range(-nd, 0))
    f1 = torch.fft.rfftn(x, s=size, dim=dims)
    f2 = f1 if x2 is None else torch.fft.rfftn(x2, s=size, dim=dims)
    spec = (f1 * f2.conj()).mean(dim=0).sum(dim=0).real.flatten()
    kbin, w, kmag = _shells(size, x.device)
    wf = w.to(spec.dtype)
    nb = int(kbin.max().item()) + 1
    ksum = torch.bincount(kbin, weights=kmag * wf, minlength=nb)
    psum = torch.bincount(kbin, weights=spec * wf, minlength=nb)
    nsum = torch.bincount(kbin, weights=wf, minlength=nb).round().to(torch.int32)
    sl = slice(1, 1 + kmax)
    n = nsum[sl]
    return ksum[sl] / n, psum[sl] / n, n


def pk(fields, fields2=None):
    """Per-sample spectra (summed over channels), stacked over the batch."""
    rows = [power(f[None], None if fields2 is None else fields2[i][None]) for i, f in enumerate(fields)]
    return tuple(torch.stack([r[j] for r in rows], dim=0) for j in range(3))


def get_ccs(fields1, fields2, full=False):
    """Cross-correlation coefficient P12 / sqrt(P11 P22), paired (default) or all pairs (full=True)."""
    ks, p11, _ = pk(fields1)
    p22 = pk(fields2)[1]
    if full:
        n = len(fields2)
        rows = [pk(f1[None].expand(n, *f1.shape), fields2)[1] for f1 in fields1]
        return ks, torch.stack(rows, dim=0) / torch.sqrt(p11[:, None] * p22[None, :])
    assert len(fields1) == len(fields2)
    return ks, pk(fields1, fields2)[1] / torch.sqrt(p11 * p22)


# ------------------------------------------------------------------------------------------------------------------
def config_fields(config):
    """(conditioning field names, K) of a config: `in_field_name` may be "A+B+C" (up to three fields); an explicit
    `conditioning_channels` that disagrees with it is a ValueError."""
    from .data import split_fields
    names = split_fields(config.get("in_field_name", "Mstar"))
    k = config.get("conditioning_channels")
    if k is not None and int(k) not in (0, len(names)):          # (0: an unconditional model, whatever field the data module also loads)
        raise ValueError(f"conditioning_channels = {k} disagrees with in_field_name = {config.get('in_field_name')!r} ({len(names)} fields)")
    return names, (len(names) if k is None else int(k))


def get_datamodule(config):
    assert "data_params" in config, "data_params not in config"
    dp = config["data_params"]
    from . import data
    names, _ = config_fields(config)
    return data.get_dataset(
        dataset_name=dp["dataset_name"], suite_name=dp.get("suite_name", "Astrid"), return_func=data.cond_return_func(len(names)),
        set_name=dp.get("set_name", "CV"), z_name=dp.get("z_name", "z_0.0"),
        channel_names=names + [config["out_field_name"]], stage=dp.get("stage", "test"),
        batch_size=dp.get("batch_size", 1), cropsize=config["cropsize"], num_workers=8, mmap=False)


def get_model(config, backend="hip", precision=None, load_ckpt=True):
    """config dict (one entry of configs.yaml) -> LightVDM, defaults as in /root/reference/src/utils.py:434-462."""
    import os
    if config["type"] != "VDM":
        if config["type"] == "SFM":
            return None                                      # as in the reference (generate_3D.py refuses SFM)
        raise ValueError(f"Unknown model type {config['type']}")
    from . import networks, vdm_model
    w_cfg, cfg_drop = guidance_knobs(config)             # (bad values: a ValueError before any model or GPU work)
    weights = weights_knob(config)
    n_values = config.get("conditioning_values", 6)
    cropsize = config.get("cropsize", 128)
    score_model = networks.CUNet(
        shape=(1, cropsize, cropsize, cropsize),
        chs=config.get("chs", [32, 64, 128, 256]),
        s_conditioning_channels=config_fields(config)[1],
        v_conditioning_dims=[] if n_values == 0 else [n_values],
        t_conditioning=True, norm_groups=8, mid_attn=False, dropout_prob=0.1,
        conv_padding_mode="circular" if cropsize == 256 else "zeros", n_attention_heads=4,
        backend=backend, precision=precision or config.get("precision", "bf16"))
    path = config.get("ckpt_path")
    ck = torch.load(path, map_location="cpu") if (load_ckpt and path and os.path.exists(path)) else None
    has_ema = isinstance(ck, dict) and ck.get("ema_state_dict") is not None
    if weights == "ema" and load_ckpt and not has_ema:
        raise ValueError(f"weights='ema' (VDM4CDM_WEIGHTS / config key weights): "
                         + (f"the checkpoint {path} holds no ema_state_dict" if ck is not None else f"there is no checkpoint ({path!r})")
                         + " - it was not trained with VDM4CDM_EMA_DECAY; use weights='raw'")
    recorded = ck.get("cfg_dropout") if isinstance(ck, dict) else None
    if w_cfg is not None:
        if cfg_drop is None:                               # by default what the checkpoint's training run dropped
            cfg_drop = recorded["cfg_drop"] if recorded else "v"
        vdm_model.check_cfg_args(0.0, cfg_drop, score_model, "get_model(w_cfg)")
        if not recorded or float(recorded["p_uncond"]) == 0.0:
            print(f"[vdm4cdm_amd] WARNING: w_cfg={w_cfg} asks for classifier-free guidance, but "
                  + ("the checkpoint records p_uncond=0" if recorded else "no checkpoint records conditioning dropout (p_uncond)")
                  + f": the network never saw the null token, its unguided branch (cfg_drop={cfg_drop!r}) is untrained", flush=True)
    vdm = vdm_model.LightVDM(score_model=score_model, draw_figure=None, gamma_max=13.3, learning_rate=3.0e-4,
                             **({} if w_cfg is None else {"w_cfg": w_cfg, "cfg_drop": cfg_drop}))
    if ck is not None and has_ema and weights != "raw":
        if weights is None:
            print(f"[vdm4cdm_amd] {path} holds EMA weights (decay {ck.get('ema', {}).get('decay')}): sampling from them "
                  "(VDM4CDM_WEIGHTS=raw for the last-step weights)", flush=True)
        vdm.load_state_dict(ck["ema_state_dict"])
    elif ck is not None:
        vdm.load_state_dict(ck["state_dict"])
    elif load_ckpt and path:
        print(f"[vdm4cdm_amd] checkpoint {path} not found: using seeded random weights (no trained weights ship with this repo)")
    return vdm


def weights_knob(config):
    """Which weights of a checkpoint a generation run samples from: $VDM4CDM_WEIGHTS / config["weights"] (the environment wins) -
    "ema" (the checkpoint's ema_state_dict; a checkpoint without one is refused), "raw" (its state_dict), or None when neither is set:
    the averaged weights if the checkpoint holds them, announced in one line, else the raw ones.  Any other value is a ValueError."""
    import os
    w = os.environ.get("VDM4CDM_WEIGHTS")
    w = config.get("weights") if w in (None, "") else w
    if w is not None and w not in ("ema", "raw"):
        raise ValueError(f"weights={w!r} (VDM4CDM_WEIGHTS / config key weights): one of 'ema', 'raw'")
    return w


def guidance_knobs(config):
    """(w_cfg or None, cfg_drop or None) of a generation run: $VDM4CDM_W_CFG / config["w_cfg"] and $VDM4CDM_CFG_DROP /
    config["cfg_drop"] (the environment wins).  Host-only; a value that is no finite number / none of "v", "s", "vs" is a ValueError."""
    import math
    import os
    from .vdm_model import CFG_DROPS
    w = os.environ.get("VDM4CDM_W_CFG")
    w = config.get("w_cfg") if w in (None, "") else w
    if w is not None:
        try:
            w = float(w)
        except (TypeError, ValueError):
            raise ValueError(f"w_cfg={w!r} is not a number (VDM4CDM_W_CFG / config key w_cfg)") from None
        if not math.isfinite(w):
            raise ValueError(f"w_cfg={w!r} must be finite (VDM4CDM_W_CFG / config key w_cfg)")
    drop = os.environ.get("VDM4CDM_CFG_DROP")
    drop = config.get("cfg_drop") if drop in (None, "") else drop
    if drop is not None and drop not in CFG_DROPS:
        raise ValueError(f"cfg_drop={drop!r} (VDM4CDM_CFG_DROP / config key cfg_drop): one of {', '.join(map(repr, CFG_DROPS))}")
    return w, drop


class MaskOperator:
    """DDNM measurement y = mask * x (inpainting): A = AT = x -> mask * x.  `mask` broadcasts to the cube batch (B, *shape).  .A / .AT
    are plain torch callables (any device); on the HIP backend get_ddnm_result(operator=) runs the fused mask kernel instead."""
    kind = "mask"

    def __init__(self, mask):
        self.mask = torch.as_tensor(mask, dtype=torch.float32)
        self._dev = {}

    def _m(self, x):
        m = self._dev.get(x.device)
        if m is None:
            m = self._dev[x.device] = self.mask.to(x.device)
        return m

    def A(self, x):
        return x * self._m(x)

    AT = A

    def check(self, shape):
        try:
            ok = tuple(torch.broadcast_shapes(tuple(self.mask.shape), tuple(shape))) == tuple(shape)
        except RuntimeError:
            ok = False
        if not ok:
            raise ValueError(f"MaskOperator: a mask of shape {tuple(self.mask.shape)} does not broadcast to the cube batch {tuple(shape)}")


class BlockMeanOperator:
    """DDNM measurement y = block-mean(x) (super-resolution): A = mean over fz x fy x fx blocks of the last three axes, AT = nearest
    up-sampling, its pseudo-inverse (A AT = I, exactly: the block sum is a pairwise tree, so equal values add without rounding).
    Each factor is 1, 2, 4 or 8.  On the HIP backend get_ddnm_result(operator=) runs the fused block-mean kernel instead."""
    kind = "blockmean"

    def __init__(self, factors):
        factors = tuple(int(f) for f in factors)
        if len(factors) != 3 or any(f not in (1, 2, 4, 8) for f in factors):
            raise ValueError(f"BlockMeanOperator: factors = {factors} (three values out of 1, 2, 4, 8)")
        self.factors = factors

    def A(self, x):
        n = 1
        for ax, f in zip((-3, -2, -1), self.factors):
            n *= f
            while f > 1:
                even = [slice(None)] * x.dim()
                odd = [slice(None)] * x.dim()
                even[ax], odd[ax] = slice(0, None, 2), slice(1, None, 2)
                x = x[tuple(even)] + x[tuple(odd)]
                f //= 2
        return x * (1.0 / n) if n > 1 else x

    def AT(self, y):
        for ax, f in zip((-3, -2, -1), self.factors):
            if f > 1:
                y = y.repeat_interleave(f, dim=ax)
        return y

    def check(self, shape):
        if len(shape) < 4 or any(d % f for d, f in zip(shape[-3:], self.factors)):
            raise ValueError(f"BlockMeanOperator: factors {self.factors} do not divide the cube {tuple(shape[-3:])}")


def get_ddnm_result(vdm, y, A=None, AT=None, n_sampling_steps=250, l=10, return_all=False, verbose=0, *, seed=None, seeds=None,
                    noises=None, operator=None, use_graph=True, stats=None, **kwargs):
    """DDNM range/null-space sampler with time travel (length l), on this package's VDM.
    Without seed / seeds / noises / operator: the reference's loop as it stands (global torch RNG, eager evaluations).
    With any of them: the seed- or noise-keyed sampler (sampling.ddnm_sample) - on the HIP backend one replayed hipGraph per network
    evaluation with the DDNM update as HIP kernels.  seeds: one int per row of y, every row a chain of its own (its result does not
    depend on the batch it sits in); seed: one stream for the whole batch; noises: every field in call order, z_1 first;
    operator: a MaskOperator / BlockMeanOperator (A and AT may then be omitted; the update is one fused kernel); generic A / AT
    run inside the captured step and must be device-only torch ops with fixed shapes (use_graph=False: the same kernels, un-captured).
    The batch is y's row count (one seed per row of y).  stats: a dict that the device loop of the HIP backend fills for tests and
    tools ({"graph", "evaluations", "allocated_before", "allocated_after"}: whether a captured step was replayed, the number of
    network evaluations, torch.cuda.memory_allocated before the first and after the last evaluation); nothing is recorded without it."""
    if seed is not None or seeds is not None or noises is not None or operator is not None:
        from .sampling import ddnm_sample
        return ddnm_sample(vdm.model, y, A, AT, operator, n_sampling_steps, l, return_all, verbose, seed, seeds, noises, use_graph,
                           vdm.device, kwargs, stats)
    if A is None or AT is None:
        raise ValueError("get_ddnm_result: give A and AT, or operator=")
    if isinstance(l, int):
        l = np.full(n_sampling_steps, l)
    l = np.asarray(l)
    assert l.ndim == 1 and len(l) == n_sampling_steps and np.issubdtype(l.dtype, np.integer) and np.all(l >= 0), \
        "l must be a non-negative integer or an integer array of length n_sampling_steps"
    dev = vdm.device
    steps = torch.linspace(1.0, 0.0, n_sampling_steps + 1, device=dev)
    z = torch.randn((y.shape[0], *vdm.model.score_model.shape), device=dev)
    ATy = AT(y)
    xs = []
    x_r = None
    with torch.no_grad():
        for i in range(n_sampling_steps):
            L = int(min(l[i], i))
            z = vdm.model.sample_zt_given_zs(zs=z, t=steps[i - L], s=steps[i])          # travel back L steps
            for j in range(L, -1, -1):
                w_z, w_x, x0, scale = vdm.model.sample_zs_given_zt(zt=z, conditioning=None, t=steps[i - j], s=steps[i + 1 - j],
                                                                   return_ddnm=True, **kwargs)
                x_r = ATy + x0 - AT(A(x0))                                              # range-space correction
                z = w_z * z + w_x * x_r + scale * torch.randn_like(z)
            if return_all:
                xs.append(x_r)
            if verbose and i % 25 == 0:
                print(f"ddnm {i}/{n_sampling_steps}", flush=True)
    return torch.stack(xs, dim=0) if return_all else x_r
