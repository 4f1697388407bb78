"""``vdm_model.VDM`` / ``vdm_model.LightVDM`` - variational diffusion model around the CUNet score network.

Mirrors the interface the reference uses for ``mltools.models.vdm_model``:
* construction ``LightVDM(score_model=, draw_figure=, gamma_min=, gamma_max=, noise_schedule=, learning_rate=)``
  (/root/reference/trainVDM3D128_c_c_from_field_name_thick_lowbatch.py:128-132, train_uc_uc_from_field_name.py:115-120)
* ``.model.score_model``, ``.model.gamma_min/gamma_max/w_cfg``, ``.model.sample_zs_given_zt(zt=, t=, s=, return_ddnm=)``,
  ``.model.sample_zt_given_zs(zs=, t=, s=)``, ``.device`` (/root/reference/src/utils.py:286-299)
* ``.draw_samples(batch_size, n_sampling_steps, verbose, return_all, **kwargs)`` (notebook frame vdm_model.py:531-557;
  call sites /root/reference/generate_3D.py:61)
* ``load_state_dict(torch.load(p)["state_dict"])`` (/root/reference/src/utils.py:468-469)
The arithmetic is spec D9-D12 of SURVEY.md section 8 (the mltools source is not in the reference tree).

On a GPU with the HIP backend the forward diffusion, the ELBO reductions and the ancestral update are the
HIP kernels K7-K9 and the denoise step is captured once in a hipGraph and replayed for every step
(per-step scalars come from a device table indexed by a device-side step counter): vdm4cdm_amd.sampling, whose names stay importable here.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _experiment
from .sampling import ChainNoise, ddnm_lengths, ddnm_sample, ddnm_schedule, hip_ddnm_sampler, hip_graph_sampler  # noqa: F401
from .sampling import check_sampler, hip_multistep_sampler, multistep_loop

DATA_NOISE = 1.0e-3
# Fused head of the HIP training step (vdm_diffuse_pack + vdm_loss_terms_rng; fused_head=0: randn -> diffuse -> pack_input, A/B)
FUSED_HEAD = bool(_experiment.get("fused_head"))


class _DiffusionLossFn(torch.autograd.Function):
    """sum_n coef_n * sum (eps_hat - eps)^2 / 2 ... via the fused HIP reduction (K8)."""

    @staticmethod
    def forward(ctx, eps_hat, x, eps, eps0, s0a0, coef, sums):
        from . import hip_ops as ops
        d = torch.empty_like(eps_hat)
        ops.loss_terms(x, eps, eps_hat.contiguous(), eps0, s0a0, coef, sums, d)
        ctx.save_for_backward(d)
        # coef_n = 2 w_n  ->  loss = sum_n w_n S_n = 0.5 sum_n coef_n S_n
        return 0.5 * (coef * sums[:, 0]).sum()

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return g * d, None, None, None, None, None, None


class _ElboFn(torch.autograd.Function):
    """(elbo, [diffusion, latent, reconstruction]) in bits/dim: K8 (fused per-sample reductions + d eps_hat) and the scalar assembly
    (vdm_elbo_assemble) - three launches; the metrics are not differentiable, d elbo / d eps_hat = coef_n (eps_hat - eps)."""

    @staticmethod
    def forward(ctx, eps_hat, x, eps, eps0, s0a0, coef, consts, rng=None):
        """rng = ((seed, stream) of eps, (seed, stream) of eps0): fields passed as None are regenerated in the kernel (fused head)."""
        from . import hip_ops as ops
        d = torch.empty_like(eps_hat)
        sums = torch.zeros(x.shape[0], 3, device=x.device)
        ops.loss_terms(x, eps, eps_hat.contiguous(), eps0, s0a0, coef, sums, d, rng=rng)
        out = ops.elbo_assemble(sums, coef, *consts)
        ctx.save_for_backward(d)
        elbo, parts = out[0], out[1:]
        ctx.mark_non_differentiable(parts)
        return elbo, parts

    @staticmethod
    def backward(ctx, g, _):
        (d,) = ctx.saved_tensors
        return g * d, None, None, None, None, None, None, None


def _cond_fields(s_c, x, K):
    """The K > 1 conditioning fields of a training batch as contiguous fp32 [B, K, D, H, W] on x's device."""
    assert s_c is not None, f"s_conditioning_channels={K} needs s_conditioning"
    s_c = s_c.to(device=x.device, dtype=torch.float32)
    assert s_c.dim() == x.dim() and s_c.shape[1] == K and s_c.shape[2:] == x.shape[2:], \
        f"s_conditioning must be [B, {K}, ...] on the grid of x, got {tuple(s_c.shape)}"
    return s_c.expand(x.shape[0], *s_c.shape[1:]).contiguous()


class _LearnedDiffuseFn(torch.autograd.Function):
    """z_t = alpha_n x + sigma_n eps of the learned schedule through the fused head (vdm_diffuse_pack: conv_in's packed input in the same
    pass; eps None: drawn in the kernel from rng = (seed, stream)).  Backward: d alpha_n = sum dz x, d sigma_n = sum dz eps (K7b, eps read
    or regenerated from the same counters); alpha / sigma are [B] tensors of torch autograd over (gamma_b, gamma_w)."""

    @staticmethod
    def forward(ctx, alpha, sigma, x, eps, rng, s_cond, dtype, keep_s=None):
        from . import hip_ops as ops
        head = ops.diffuse_pack_fields if (s_cond is not None and s_cond.shape[1] > 1) else ops.diffuse_pack      # [B, K, ...], K = 2, 3
        kw = {} if keep_s is None else {"keep_s": keep_s}          # conditioning dropout: the dropped rows' planes are +0 (p_uncond)
        z_t, xin = head(x, s_cond, alpha.detach().contiguous(), sigma.detach().contiguous(), dtype, eps=eps, seed=rng[0],
                        stream_id=rng[1], want_z=True, **kw)
        ctx.save_for_backward(x, eps)
        ctx.rng = rng
        ctx.mark_non_differentiable(xin)
        return z_t, xin

    @staticmethod
    def backward(ctx, dz, _):
        from . import hip_ops as ops
        x, eps = ctx.saved_tensors
        if dz is None:
            return (None,) * 8
        sums = ops.schedule_grad_sums(dz.contiguous(), x, eps, *ctx.rng)
        return sums[:, 0], sums[:, 1], None, None, None, None, None, None


class _LearnedElboFn(torch.autograd.Function):
    """K8 for the learned schedule: (diffusion loss 0.5 sum_n coef_n S_n, sums [B, 3]).  coef_n = |w| bpd / B is an input, so that
    d loss / d coef_n = S_n / 2 reaches gamma_w (the diffusion weight gamma'(t) = |w|).  The kernel runs with sigma0/alpha0 = 1:
    sums[:, 2] = sum eps0^2, which the reconstruction term scales by e^{gamma(0)} (= (sigma0/alpha0)^2) in torch."""

    @staticmethod
    def forward(ctx, eps_hat, coef, x, eps, eps0, rng):
        from . import hip_ops as ops
        c = coef.detach().contiguous()
        d = torch.empty_like(eps_hat)
        sums = torch.zeros(x.shape[0], 3, device=x.device)
        ops.loss_terms(x, eps, eps_hat.contiguous(), eps0, 1.0, c, sums, d, rng=rng)
        ctx.save_for_backward(d, sums)
        ctx.mark_non_differentiable(sums)
        return 0.5 * (c * sums[:, 0]).sum(), sums

    @staticmethod
    def backward(ctx, g, _):
        d, sums = ctx.saved_tensors
        return g * d, 0.5 * g * sums[:, 0], None, None, None, None


CFG_DROPS = ("v", "s", "vs")
COND_KEEP_SEED_SALT = 0xCFD05EED          # cond_keep_seed = torch.initial_seed() ^ this: a stream of its own, not train_generator's
_GOLDEN64, _MASK64 = 0x9E3779B97F4A7C15, (1 << 64) - 1


class CfgConditioningError(ValueError, AssertionError):
    """Guidance asked to mask a conditioning that was not passed (a ValueError; also an AssertionError, which this case raised before)."""


def check_cfg_args(p_uncond=0.0, cfg_drop="v", score_model=None, who="VDM"):
    """Validates (p_uncond, cfg_drop) on the host; with a network also that it has the conditionings cfg_drop names.  Returns
    (float p_uncond, cfg_drop)."""
    try:
        p = float(p_uncond)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: p_uncond={p_uncond!r} is not a number") from None
    if not (math.isfinite(p) and 0.0 <= p <= 1.0):
        raise ValueError(f"{who}: p_uncond={p_uncond!r} must be a finite number in [0, 1]")
    if cfg_drop not in CFG_DROPS:
        raise ValueError(f"{who}: cfg_drop={cfg_drop!r} (one of {', '.join(map(repr, CFG_DROPS))})")
    if score_model is not None:
        if "v" in cfg_drop and not getattr(score_model, "v_conditioning_dims", None):
            raise ValueError(f"{who}: cfg_drop={cfg_drop!r} drops the vector conditionings, but the network has no v_conditioning_dims")
        if "s" in cfg_drop and not getattr(score_model, "s_conditioning_channels", 0):
            raise ValueError(f"{who}: cfg_drop={cfg_drop!r} drops the conditioning fields, but the network has s_conditioning_channels=0")
    return p, cfg_drop


def _rows(keep, t):
    return keep.view((-1,) + (1,) * (t.dim() - 1))


class _MaskRowsFn(torch.autograd.Function):
    """vdm_mask_rows with its gradient: rows with keep == 0 are +0 in the output and in the gradient (a select in both directions)."""

    @staticmethod
    def forward(ctx, v, keep):
        from . import hip_ops as ops
        ctx.save_for_backward(keep)
        return ops.mask_rows(v.contiguous(), keep)

    @staticmethod
    def backward(ctx, g):
        from . import hip_ops as ops
        g = g.contiguous()
        return ops.mask_rows(g, ctx.saved_tensors[0], out=g), None


class _MaskGradFn(torch.autograd.Function):
    """Identity whose gradient is row-masked: for a conditioning field the fused head has already dropped (its forward never reads the
    dropped rows), so that the ds planes K1t returns are +0 in those rows."""

    @staticmethod
    def forward(ctx, s, keep):
        ctx.save_for_backward(keep)
        return s.view_as(s)

    @staticmethod
    def backward(ctx, g):
        from . import hip_ops as ops
        g = g.contiguous()
        return ops.mask_rows(g, ctx.saved_tensors[0], out=g), None


class VDM(nn.Module):
    def __init__(self, score_model, noise_schedule="fixed_linear", gamma_min=-13.3, gamma_max=13.3,
                 antithetic_time_sampling=True, data_noise=DATA_NOISE, w_cfg=None, p_uncond=0.0, cfg_drop="v"):
        """p_uncond / cfg_drop: classifier-free guidance training - in training mode every global row sees, with probability p_uncond
        and on its own, the null token (zeros) instead of the conditioning(s) cfg_drop names ("v": the vector conditionings, "s": the
        conditioning fields, all K planes, "vs": both, the same rows).  With w_cfg the unguided half of the sampler's batch-doubled
        forward masks the same conditioning(s).  p_uncond == 0: the training step is exactly the one without the feature."""
        super().__init__()
        assert noise_schedule in ("fixed_linear", "learned_linear")
        self.p_uncond, self.cfg_drop = check_cfg_args(p_uncond, cfg_drop)
        if self.p_uncond > 0 or w_cfg is not None:     # (the feature is in use: the network must have what cfg_drop names)
            check_cfg_args(p_uncond, cfg_drop, score_model)
        self.last_cond_keep = None               # [B] fp32 {0, 1} of the latest training step that drew one (a graph replay refreshes it)
        self._cond_keep_seed = None
        self._cond_keep_calls = 0                # eager steps: mixed into the seed on the host (a captured step: hip_ops.SEED_STEP)
        self.score_model = score_model
        self.noise_schedule = noise_schedule
        self.gamma_min = float(gamma_min)
        self.gamma_max = float(gamma_max)
        self.antithetic_time_sampling = antithetic_time_sampling
        self.data_noise = float(data_noise)
        self.w_cfg = w_cfg
        if noise_schedule == "learned_linear":                   # D9: gamma(t) = b + |w| t
            self.gamma_b = nn.Parameter(torch.tensor(self.gamma_min))
            self.gamma_w = nn.Parameter(torch.tensor(self.gamma_max - self.gamma_min))
        self._graph = None

    # ---------------------------------------------------------------- schedule (D9)
    def gamma(self, t):
        if self.noise_schedule == "learned_linear":
            return self.gamma_b + self.gamma_w.abs() * t
        return self.gamma_min + (self.gamma_max - self.gamma_min) * t

    def dgamma_dt(self, t):
        if self.noise_schedule == "learned_linear":
            return self.gamma_w.abs() * torch.ones_like(t)
        return (self.gamma_max - self.gamma_min) * torch.ones_like(t)

    @staticmethod
    def alpha(g):
        return torch.sqrt(torch.sigmoid(-g))

    @staticmethod
    def sigma(g):
        return torch.sqrt(torch.sigmoid(g))

    def _hip(self, ref):
        return getattr(self.score_model, "backend", None) == "hip" and ref.is_cuda

    # ---------------------------------------------------------------- score
    def get_pred_noise(self, zt, gamma_t, **kwargs):
        """notebook frame vdm_model.py:309-327."""
        t = (gamma_t - self.gamma_min) / (self.gamma_max - self.gamma_min)
        if self.w_cfg is None or self.training:
            return self.score_model(zt, t=t, **kwargs)
        eps_c, eps_u = self._cfg_pair(zt, t, kwargs)
        return (1.0 + self.w_cfg) * eps_c - self.w_cfg * eps_u

    @staticmethod
    def cfg_mask(v_conditionings):
        """The "masked out" vector conditionings of the unguided branch (frame vdm_model.py:327: "Need v_conditionings to mask out";
        the masking value is not in the reference tree - [INFERRED] zeros, the usual null token of a vector conditioning)."""
        return [torch.zeros_like(v) for v in v_conditionings]

    def _cfg_check(self, kwargs):
        """(mask v?, mask s?) of the unguided half under w_cfg; raises before any GPU work when what cfg_drop names was not passed."""
        drop_v, drop_s = "v" in self.cfg_drop, "s" in self.cfg_drop
        check_cfg_args(self.p_uncond, self.cfg_drop, self.score_model, "w_cfg")
        if drop_v and kwargs.get("v_conditionings") is None:
            raise CfgConditioningError(f"Need v_conditionings to mask out (w_cfg with cfg_drop={self.cfg_drop!r})")
        if drop_s and kwargs.get("s_conditioning") is None:
            raise CfgConditioningError(f"Need s_conditioning to mask out (w_cfg with cfg_drop={self.cfg_drop!r})")
        return drop_v, drop_s

    # ---------------------------------------------------------------- conditioning dropout (classifier-free guidance training)
    @property
    def cond_keep_seed(self):
        """Philox seed of the keep stream: derived once per model from torch.initial_seed() and a constant - nothing is drawn from
        train_generator, so the times, noise fields and dropout masks of a run do not depend on p_uncond."""
        if self._cond_keep_seed is None:
            self._cond_keep_seed = (torch.initial_seed() ^ COND_KEEP_SEED_SALT) & 0x7fffffffffffffff
        return self._cond_keep_seed

    def _draw_keep(self, B, device, hip):
        """The [B] fp32 keep of this training step (None: eval mode or p_uncond == 0 - nothing is drawn or launched).  Row i of rank r is
        global row r B + i.  HIP: one vdm_cond_keep launch, Philox counters (row, 0xCFD0), key = cond_keep_seed mixed with the step - the
        device counter of a captured step, else this model's host call counter.  Torch backend: torch.rand(B) > p from the rank's
        noise generator (not the Philox rows)."""
        if not (self.training and self.p_uncond > 0.0):
            return None
        rank, _ = self._rank_world()
        if hip:
            from . import hip_ops as ops
            seed = self.cond_keep_seed
            if ops.SEED_STEP is None:
                seed = (seed + (self._cond_keep_calls & 0xFFFFFFFF) * _GOLDEN64) & _MASK64
                self._cond_keep_calls += 1
            keep = ops.cond_keep(self.p_uncond, seed, B, device, row0=rank * B)
        else:
            keep = (torch.rand(B, device=device, generator=self._rank_noise_gen(device, rank)) > self.p_uncond).to(torch.float32)
        self.last_cond_keep = keep
        return keep

    def _drop_conditioning(self, kwargs, keep, x, hip, head_drops_s=False):
        """kwargs with the conditionings cfg_drop names replaced by their row-masked copies (null token: zeros).  head_drops_s: the fused
        head writes the dropped rows' planes itself (keep_s) and the network never reads s_conditioning - only its gradient is masked."""
        kw, B = dict(kwargs), x.shape[0]
        if "v" in self.cfg_drop and kw.get("v_conditionings"):
            vs = []
            for v in kw["v_conditionings"]:
                v = v.to(device=x.device, dtype=torch.float32)
                v = v.expand(B, *v.shape[1:]) if v.shape[0] != B else v
                vs.append(_MaskRowsFn.apply(v, keep) if hip else torch.where(_rows(keep, v) != 0, v, torch.zeros_like(v)))
            kw["v_conditionings"] = vs
        if "s" in self.cfg_drop and kw.get("s_conditioning") is not None:
            s = kw["s_conditioning"].to(device=x.device, dtype=torch.float32)
            s = s.expand(B, *s.shape[1:]) if s.shape[0] != B else s
            if not hip:
                kw["s_conditioning"] = torch.where(_rows(keep, s) != 0, s, torch.zeros_like(s))
            elif not head_drops_s:
                kw["s_conditioning"] = _MaskRowsFn.apply(s, keep)
            elif s.requires_grad:
                kw["s_conditioning"] = _MaskGradFn.apply(s, keep)
        return kw

    def _cfg_pair(self, zt, t, kwargs):
        """Classifier-free guidance (notebook frame vdm_model.py:318-327): conditional and v-masked noise estimates from ONE
        batch-doubled UNet forward (rows 0..B-1 with the given v_conditionings, rows B..2B-1 with them masked)."""
        drop_v, drop_s = self._cfg_check(kwargs)
        B = zt.shape[0]
        kw = dict(kwargs)
        if kwargs.get("v_conditionings") is not None:
            vs = [v.to(zt.device).expand(B, *v.shape[1:]) if v.shape[0] != B else v.to(zt.device) for v in kwargs["v_conditionings"]]
            kw["v_conditionings"] = [torch.cat([v, m], dim=0) for v, m in zip(vs, self.cfg_mask(vs) if drop_v else vs)]
        if kw.get("s_conditioning") is not None:
            sc = kw["s_conditioning"]
            sc = sc.expand(B, *sc.shape[1:]) if sc.shape[0] != B else sc
            kw["s_conditioning"] = torch.cat([sc, torch.zeros_like(sc) if drop_s else sc], dim=0)      # (cfg_drop "s": the zero cube)
        t2 = torch.cat([t.expand(B), t.expand(B)]) if torch.is_tensor(t) else t
        eps = self.score_model(torch.cat([zt, zt], dim=0), t=t2, **kw)
        return eps[:B], eps[B:]

    # ---------------------------------------------------------------- loss (D10)
    @staticmethod
    def _rank_world():
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
        return 0, 1

    def _rank_noise_gen(self, device, rank):
        g = getattr(self, "_noise_gen", None)
        if g is None or g.device != torch.device(device) or self._noise_gen_key != (torch.initial_seed(), rank):
            g = torch.Generator(device=device)
            g.manual_seed((torch.initial_seed() + 0x9E3779B97F4A7C15 * (rank + 1)) & 0x7fffffffffffffff)
            self._noise_gen, self._noise_gen_key = g, (torch.initial_seed(), rank)
        return g

    def sample_times(self, B, device):
        return stratified_times(B, device, self.antithetic_time_sampling)

    def get_loss(self, x, times=None, eps=None, eps0=None, **kwargs):
        """Continuous-time ELBO in bits/dim.  Returns (loss, metrics dict)."""
        B = x.shape[0]
        numel = x[0].numel()
        bpd = 1.0 / (numel * math.log(2.0))
        x = x.to(torch.float32).contiguous()
        hip = self._hip(x)
        keep = self._draw_keep(B, x.device, hip)      # conditioning dropout: None unless training with p_uncond > 0
        if hip and self.noise_schedule == "learned_linear":
            return self._hip_learned_loss(x, times, eps, eps0, numel, bpd, kwargs, keep)
        if not hip:
            if times is None:
                times = self.sample_times(B, x.device)
            g_t = self.gamma(times)
        # 0-dim CPU tensors act as scalars (no device sync for the fixed schedule)
        # (fp64: var1 - log(var1) - 1 ~ 1e-12 cancels catastrophically in fp32)
        g0 = self.gamma(torch.zeros((), dtype=torch.float64))
        g1 = self.gamma(torch.ones((), dtype=torch.float64))
        var1 = torch.sigmoid(g1)
        a0, s0 = self.alpha(g0), self.sigma(g0)
        bc = (B,) + (1,) * (x.dim() - 1)
        if hip:
            from . import hip_ops as ops
            rank, world = self._rank_world()              # (Philox stream id = 2*rank + {1,2}: different noise fields per rank)
            # Fused head: with no noise supplied, eps and eps0 are never materialised - K7 draws eps from its Philox
            # counters while it forms z_t and writes conv_in's packed input in the same pass, K8 regenerates both fields from the same
            # counters.  The host draws the two seeds exactly as the unfused path does (same generator state -> same noise fields).
            sm = self.score_model
            fuse = (FUSED_HEAD and eps is None and eps0 is None and numel % 4 == 0 and (self.w_cfg is None or self.training)
                    and x.dim() == 5 and getattr(sm, "s_conditioning_channels", 0) <= 3)
            rng = None
            if fuse:
                rng = ((noise_seed(), 2 * rank + 1), (noise_seed(), 2 * rank + 2))
            else:
                if eps is None:
                    eps = ops.randn(torch.empty_like(x), noise_seed(), 2 * rank + 1)
                if eps0 is None:
                    eps0 = ops.randn(torch.empty_like(x), noise_seed(), 2 * rank + 2)
            # the scalar side of the step in ONE launch: time grid (stratified over the global batch), alpha_t, sigma_t, the per-sample
            # loss weight 2 w_n = gamma'(t) bpd / B and the network's normalised time - no ATen launch between the noise draw and K7
            if times is None and self.antithetic_time_sampling and ops.SEED_STEP is not None:
                # graph-captured step (trainer.GraphedTrainStep): u0 comes out of the kernel, from a fixed seed and the device step counter
                if getattr(self, "_graph_seed", None) is None:
                    self._graph_seed = noise_seed()
                sc = ops.train_scalars(B, x.device, rank, world, self.gamma_min, self.gamma_max, bpd / B, seed=self._graph_seed)
            elif times is None and self.antithetic_time_sampling:
                u0 = torch.rand(1, device=x.device, generator=train_generator(x.device))
                sc = ops.train_scalars(B, x.device, rank, world, self.gamma_min, self.gamma_max, bpd / B, u0=u0)
            else:
                if times is None:
                    times = self.sample_times(B, x.device)
                sc = ops.train_scalars(B, x.device, 0, 1, self.gamma_min, self.gamma_max, bpd / B,
                                       times=times.to(device=x.device, dtype=torch.float32).contiguous())
            if fuse:
                s_c = kwargs.get("s_conditioning") if sm.s_conditioning_channels else None
                assert s_c is not None or not sm.s_conditioning_channels, "s_conditioning_channels=1 needs s_conditioning"
                dt = torch.bfloat16 if sm.precision == "bf16" else torch.float32
                # conditioning dropout of the fields: the head writes +0 for the dropped rows (keep_s); none: today's launches
                hk = {"keep_s": keep} if (keep is not None and "s" in self.cfg_drop and s_c is not None) else {}
                if sm.s_conditioning_channels > 1:         # K = 2, 3 conditioning fields: the same head with K planes
                    s_c = _cond_fields(s_c, x, sm.s_conditioning_channels)
                    z_t, xin = ops.diffuse_pack_fields(x, s_c, sc[1], sc[2], dt, seed=rng[0][0], stream_id=rng[0][1], want_z=True, **hk)
                else:
                    if s_c is not None:
                        s_c = s_c.to(device=x.device, dtype=torch.float32).expand(x.shape).contiguous()
                    z_t, xin = ops.diffuse_pack(x, s_c, sc[1], sc[2], dt, seed=rng[0][0], stream_id=rng[0][1], want_z=True, **hk)
                if keep is not None:
                    kwargs = self._drop_conditioning(kwargs, keep, x, True, head_drops_s=True)
                eps_hat = self.score_model(z_t, t=sc[4], _packed_input=xin, **kwargs)
            else:
                if keep is not None:
                    kwargs = self._drop_conditioning(kwargs, keep, x, True)
                z_t = ops.diffuse(x, eps.contiguous(), sc[1], sc[2])
                if self.w_cfg is None or self.training:    # get_pred_noise's plain branch, t_norm straight from the scalar kernel
                    eps_hat = self.score_model(z_t, t=sc[4], **kwargs)
                else:
                    eps_hat = self.get_pred_noise(z_t, self.gamma(sc[0]), **kwargs)
            dn = self.data_noise
            consts = (float(0.5 * numel * (var1 - torch.log(var1) - 1.0) * bpd), float(0.5 * (1.0 - var1) * bpd),
                      float(0.5 / dn ** 2 * bpd), float(numel * (math.log(dn) + 0.5 * math.log(2 * math.pi)) * bpd))
            loss, parts = _ElboFn.apply(eps_hat, x, eps, None if eps0 is None else eps0.contiguous(), float(s0 / a0), sc[3], consts, rng)
            metrics = {"elbo": loss.detach(), "diffusion_loss": parts[0], "latent_loss": parts[1], "reconstruction_loss": parts[2]}
            return loss, metrics
        else:
            red = tuple(range(1, x.dim()))
            rank, world = self._rank_world()
            if eps is None or eps0 is None:                    # torch backend: a per-rank generator (seed ^ rank), never the global one
                g = self._rank_noise_gen(x.device, rank)
                eps = torch.randn(x.shape, device=x.device, generator=g) if eps is None else eps
                eps0 = torch.randn(x.shape, device=x.device, generator=g) if eps0 is None else eps0
            z_t = self.alpha(g_t).view(bc) * x + self.sigma(g_t).view(bc) * eps
            if keep is not None:
                kwargs = self._drop_conditioning(kwargs, keep, x, False)
            eps_hat = self.get_pred_noise(z_t, g_t, **kwargs)
            diff = (0.5 * self.dgamma_dt(times) * ((eps - eps_hat) ** 2).sum(red)).mean() * bpd
            sum_x2 = (x ** 2).sum(red)
            sum_r2 = (((s0 / a0).float() * eps0) ** 2).sum(red)
        latent = (0.5 * ((numel * (var1 - torch.log(var1) - 1.0)).float() + (1.0 - var1).float() * sum_x2)).mean() * bpd
        recons = (0.5 * sum_r2 / self.data_noise ** 2
                  + numel * (math.log(self.data_noise) + 0.5 * math.log(2 * math.pi))).mean() * bpd
        loss = diff + latent + recons
        metrics = {"elbo": loss.detach(), "diffusion_loss": diff.detach(), "latent_loss": latent.detach(),
                   "reconstruction_loss": recons.detach()}
        return loss, metrics

    def _hip_learned_loss(self, x, times, eps, eps0, numel, bpd, kwargs, keep=None):
        """get_loss of noise_schedule="learned_linear" on the HIP backend.  The activation-sized work is the fixed-linear path's kernels
        (fused head K7, K8) plus the network's input gradients (K1t dz, K6i dL/dt_norm) and K7b; the [B]-sized scalar side - gamma_t,
        alpha_t, sigma_t, t_norm, the diffusion weight |w| and the latent / reconstruction terms - is torch autograd over (gamma_b,
        gamma_w), in fp64 where the latent term cancels.  No host synchronisation."""
        from . import hip_ops as ops
        B, dev, sm = x.shape[0], x.device, self.score_model
        assert x.dim() == 5 and numel % 4 == 0, "the HIP learned-linear step needs 3D cubes with a multiple of 4 voxels"
        rank, world = self._rank_world()
        # noise: the seeds are drawn as on the fixed-linear path; a supplied field is read, a missing one drawn in the kernels
        rng_e = (noise_seed(), 2 * rank + 1) if eps is None else (0, 0)
        rng_0 = (noise_seed(), 2 * rank + 2) if eps0 is None else (0, 0)
        if times is None and self.antithetic_time_sampling:          # the fixed path's time grid (stratified over the global batch)
            u0 = torch.rand(1, device=dev, generator=train_generator(dev))
            times = ops.train_scalars(B, dev, rank, world, self.gamma_min, self.gamma_max, bpd / B, u0=u0)[0]
        elif times is None:
            times = self.sample_times(B, dev)
        times = times.to(device=dev, dtype=torch.float32).reshape(B)
        wabs = self.gamma_w.abs()
        g_t = self.gamma_b + wabs * times
        t_norm = (g_t - self.gamma_min) / (self.gamma_max - self.gamma_min)
        s_c = kwargs.get("s_conditioning") if sm.s_conditioning_channels else None
        if sm.s_conditioning_channels > 1:
            s_c = _cond_fields(s_c, x, sm.s_conditioning_channels)
        elif s_c is not None:
            s_c = s_c.to(device=dev, dtype=torch.float32).expand(x.shape).contiguous()
        dt = torch.bfloat16 if sm.precision == "bf16" else torch.float32
        keep_s = keep if (keep is not None and "s" in self.cfg_drop and s_c is not None) else None      # (None: today's launches)
        z_t, xin = _LearnedDiffuseFn.apply(self.alpha(g_t), self.sigma(g_t), x, None if eps is None else eps.contiguous(), rng_e, s_c, dt,
                                           *(() if keep_s is None else (keep_s,)))
        if keep is not None:
            kwargs = self._drop_conditioning(kwargs, keep, x, True, head_drops_s=True)
        if self.w_cfg is None or self.training:
            eps_hat = sm(z_t, t=t_norm, _packed_input=xin, **kwargs)
        else:
            eps_hat = self.get_pred_noise(z_t, g_t, **kwargs)
        coef = (wabs * (bpd / B)).expand(B)                          # 2 w_n = gamma'(t) bpd / B
        diff, sums = _LearnedElboFn.apply(eps_hat, coef, x, None if eps is None else eps.contiguous(),
                                          None if eps0 is None else eps0.contiguous(), (rng_e, rng_0))
        g0 = self.gamma_b.double()
        var1 = torch.sigmoid(g0 + self.gamma_w.double().abs())      # (fp64: var1 - log(var1) - 1 ~ 1e-12 cancels in fp32)
        s = sums.double()
        latent = (0.5 * (numel * (var1 - torch.log(var1) - 1.0) + (1.0 - var1) * s[:, 1])).mean() * bpd
        dn = self.data_noise
        recons = (0.5 * torch.exp(g0) * s[:, 2] / dn ** 2 + numel * (math.log(dn) + 0.5 * math.log(2 * math.pi))).mean() * bpd
        loss = diff + (latent + recons).float()
        metrics = {"elbo": loss.detach(), "diffusion_loss": diff.detach(), "latent_loss": latent.detach().float(),
                   "reconstruction_loss": recons.detach().float()}
        return loss, metrics

    # ---------------------------------------------------------------- sampler (D12)
    def _as_t(self, v, ref):
        return torch.as_tensor(v, dtype=torch.float32, device=ref.device)

    def sample_zs_given_zt(self, zt, t, s, return_ddnm=False, conditioning=None, **kwargs):
        """One ancestral step t -> s (notebook frame vdm_model.py:370-378).  `conditioning` is accepted and
        ignored: /root/reference/src/utils.py:296 still passes the pre-CUNet kwarg ``conditioning=None``."""
        t, s = self._as_t(t, zt), self._as_t(s, zt)
        gamma_t, gamma_s = self.gamma(t), self.gamma(s)
        c = -torch.expm1(gamma_s - gamma_t)
        alpha_t, alpha_s = self.alpha(gamma_t), self.alpha(gamma_s)
        sigma_t, sigma_s = self.sigma(gamma_t), self.sigma(gamma_s)
        pred_noise = self.get_pred_noise(zt=zt, gamma_t=gamma_t, **kwargs)
        if not return_ddnm:
            mean = alpha_s / alpha_t * (zt - c * sigma_t * pred_noise)
            scale = sigma_s * torch.sqrt(c)
            return mean + scale * torch.randn_like(zt)
        x_0t = (zt - sigma_t * pred_noise) / alpha_t
        return (alpha_s / alpha_t) * (1.0 - c), alpha_s * c, x_0t, sigma_s * torch.sqrt(c)

    def sample_zt_given_zs(self, zs, t, s, noise=None):
        """Forward diffusion s -> t (/root/reference/src/utils.py:294); `noise`: the field to use instead of a randn_like draw."""
        t, s = self._as_t(t, zs), self._as_t(s, zs)
        gamma_t, gamma_s = self.gamma(t), self.gamma(s)
        alpha_ts = self.alpha(gamma_t) / self.alpha(gamma_s)
        var = torch.sigmoid(gamma_t) - alpha_ts ** 2 * torch.sigmoid(gamma_s)
        return alpha_ts * zs + torch.sqrt(var) * (torch.randn_like(zs) if noise is None else noise)

    def _gamma_grid(self, n_sampling_steps):
        """gamma in host fp64 on the fp32 time grid ``linspace(1, 0, n+1)`` (/root/reference/src/utils.py:286), either schedule."""
        steps = torch.linspace(1.0, 0.0, n_sampling_steps + 1).double()
        with torch.no_grad():
            if self.noise_schedule == "learned_linear":
                return (self.gamma_b.double().cpu() + self.gamma_w.abs().double().cpu() * steps)
            return self.gamma_min + (self.gamma_max - self.gamma_min) * steps

    def ddnm_tables(self, n_sampling_steps, travel_lengths=None):
        """Host fp64 tables of the DDNM sampler, computed like step_table.  coef [n, 8]: row k (t = steps[k], s = steps[k+1]) =
        {1/alpha_t, sigma_t, w_z = (alpha_s/alpha_t)(1-c), w_x = alpha_s c, scale = sigma_s sqrt(c), t_norm, 0, 0} - the DDNM form of
        sample_zs_given_zt(return_ddnm=True).  With travel_lengths (L of every outer step) also travel [n, 2]: row i =
        {alpha_t/alpha_s, sqrt(sigma_t^2 - (alpha_t/alpha_s)^2 sigma_s^2)} for t = steps[i-L], s = steps[i] (sample_zt_given_zs)."""
        g = self._gamma_grid(n_sampling_steps)
        g_t, g_s = g[:-1], g[1:]
        c = -torch.expm1(g_s - g_t)
        a_t, a_s = torch.sqrt(torch.sigmoid(-g_t)), torch.sqrt(torch.sigmoid(-g_s))
        s_t, s_s = torch.sqrt(torch.sigmoid(g_t)), torch.sqrt(torch.sigmoid(g_s))
        t_norm = (g_t - self.gamma_min) / (self.gamma_max - self.gamma_min)
        zero = torch.zeros_like(c)
        coef = torch.stack([1.0 / a_t, s_t, (a_s / a_t) * (1.0 - c), a_s * c, s_s * torch.sqrt(c), t_norm, zero, zero], dim=1)
        if travel_lengths is None:
            return coef
        i = torch.arange(n_sampling_steps)
        gt, gs = g[i - torch.as_tensor(list(travel_lengths), dtype=torch.int64)], g[i]
        a_ts = torch.sqrt(torch.sigmoid(-gt)) / torch.sqrt(torch.sigmoid(-gs))
        var = torch.sigmoid(gt) - a_ts ** 2 * torch.sigmoid(gs)
        return coef, torch.stack([a_ts, torch.sqrt(var)], dim=1)

    def step_table(self, n_sampling_steps):
        """Host fp64 table [n, 4] = {alpha_s/alpha_t, c*sigma_t, sigma_s*sqrt(c), t_norm} on the fp32 time grid
        ``linspace(1, 0, n+1)`` (/root/reference/src/utils.py:286)."""
        g = self._gamma_grid(n_sampling_steps)
        g_t, g_s = g[:-1], g[1:]
        c = -torch.expm1(g_s - g_t)
        a_t, a_s = torch.sqrt(torch.sigmoid(-g_t)), torch.sqrt(torch.sigmoid(-g_s))
        s_t, s_s = torch.sqrt(torch.sigmoid(g_t)), torch.sqrt(torch.sigmoid(g_s))
        t_norm = (g_t - self.gamma_min) / (self.gamma_max - self.gamma_min)
        return torch.stack([a_s / a_t, c * s_t, s_s * torch.sqrt(c), t_norm], dim=1)

    def multistep_table(self, n_sampling_steps, order=2, lower_order_final=True):
        """Host fp64 table [n, 8] = {e_z, e_e, w_z, w_x, w_p, t_norm, 0, 0} of the deterministic multistep sampler (K9m), computed like
        step_table on the same grid; row i goes from t = steps[i] to s = steps[i+1].  DPM-Solver++(2M) (Lu et al. 2022) with the data
        prediction x_hat = (z - sigma_t eps_hat) / alpha_t = e_z z + e_e eps_hat as the modelled quantity: with lambda = log(alpha /
        sigma) = -gamma / 2, h = lambda_s - lambda_t and B = alpha_s (1 - exp(-h)),
            first order (DDIM):  z_s = (sigma_s / sigma_t) z + B x_hat
            second order (2M):   z_s = (sigma_s / sigma_t) z + B ((1 + 1/(2r)) x_hat - (1/(2r)) x_hat_prev),   r = h_prev / h
        Row 0 is first order (no history), every row with order=1, and the last row with lower_order_final (the usual guard of few-step
        chains: the last step ends at the largest log-SNR).  A first-order row has w_p = 0 exactly."""
        if order not in (1, 2):
            raise ValueError(f"multistep_table: order={order!r} (1 or 2)")
        n = n_sampling_steps
        g = self._gamma_grid(n)
        g_t, g_s = g[:-1], g[1:]
        a_t, a_s = torch.sqrt(torch.sigmoid(-g_t)), torch.sqrt(torch.sigmoid(-g_s))
        s_t, s_s = torch.sqrt(torch.sigmoid(g_t)), torch.sqrt(torch.sigmoid(g_s))
        h = 0.5 * (g_t - g_s)                                # lambda_s - lambda_t
        B = a_s * (-torch.expm1(-h))
        second = torch.zeros(n, dtype=torch.bool)
        if order == 2:
            second[1:n - 1 if lower_order_final else n] = True
        r = torch.ones_like(h)
        r[1:] = h[:-1] / h[1:]                               # from the grid itself (fp32 linspace), not assumed to be 1
        half = torch.where(second, 0.5 / r, torch.zeros_like(h))
        t_norm = (g_t - self.gamma_min) / (self.gamma_max - self.gamma_min)
        zero = torch.zeros_like(h)
        return torch.stack([1.0 / a_t, -s_t / a_t, s_s / s_t, B * (1.0 + half), -B * half, t_norm, zero, zero], dim=1)

    def _multistep_sample(self, z, n_sampling_steps, order, lower_order_final, return_all, verbose, use_graph, kwargs):
        """The deterministic samplers ("ddim": order 1, "dpm2m": order 2) from z_1 = z: the device loop on the HIP backend, the same
        table and update as a Python loop in torch fp32 otherwise."""
        coef = self.multistep_table(n_sampling_steps, order, lower_order_final)
        if self._hip(z):
            cfg = self.w_cfg is not None and not self.training
            if cfg:
                self._cfg_check(kwargs)
            return hip_multistep_sampler(self.score_model, z, coef.to(device=z.device, dtype=torch.float32).contiguous(), verbose,
                                         use_graph, kwargs.get("s_conditioning"), list(kwargs.get("v_conditionings") or []),
                                         w_cfg=float(self.w_cfg) if cfg else None, mask_fn=self.cfg_mask, return_all=return_all, cfg_drop=self.cfg_drop)
        steps = torch.linspace(1.0, 0.0, n_sampling_steps + 1, device=z.device)
        return multistep_loop(coef, z, lambda i, zt: self.get_pred_noise(zt=zt, gamma_t=self.gamma(steps[i]), **kwargs), return_all)

    @torch.no_grad()
    def sample(self, batch_size, n_sampling_steps, device, z=None, return_all=False, verbose=False,
               noises=None, seed=None, use_graph=True, seeds=None, sampler="ancestral", lower_order_final=True, **kwargs):
        """Ancestral sampling (notebook frame vdm_model.py:429-442).  `noises` (optional list of n tensors) and
        `seed` make a chain reproducible; on the HIP backend the step is a replayed hipGraph.
        `seeds` (one int per row): every row is a chain of its own, keyed by its seed wherever it sits in the batch - row r draws z_1
        and its step noise exactly as a batch-1 chain with seed=seeds[r] does (a supplied z: the seeds key the step noise only).
        `seed` with batch_size > 1 keeps its meaning of one stream for the whole batch.
        `sampler`: "ancestral" (the default: the stochastic chain above), or a deterministic solver of the probability-flow ODE on the
        same grid - "ddim" (first order) or "dpm2m" (DPM-Solver++(2M), second order, one field of history and no extra network
        evaluation; multistep_table; `lower_order_final`: its last step is first order).  They draw no step noise: seed / seeds / z
        key or supply z_1 exactly as above, noises= is an error.  Everything else in **kwargs goes to the network."""
        check_sampler(sampler)
        if sampler != "ancestral" and noises is not None:
            raise ValueError(f"sample: noises= with sampler={sampler!r}: a deterministic sampler draws no step noise (z= supplies z_1)")
        noise = ChainNoise("sample", batch_size, self.score_model.shape, device, seed, seeds, noises)
        z = noise.z1(z)
        if sampler != "ancestral":
            return self._multistep_sample(z, n_sampling_steps, 1 if sampler == "ddim" else 2, lower_order_final, return_all, verbose,
                                          use_graph, kwargs)
        if self._hip(z):                                   # (return_all: the same captured step, z copied out after every replay)
            coef = self.step_table(n_sampling_steps).to(device=z.device, dtype=torch.float32).contiguous()
            cfg = self.w_cfg is not None and not self.training
            if cfg:
                self._cfg_check(kwargs)
            return hip_graph_sampler(self.score_model, z, coef, noise, verbose, use_graph, kwargs.get("s_conditioning"),
                                     list(kwargs.get("v_conditionings") or []), w_cfg=float(self.w_cfg) if cfg else None,
                                     mask_fn=self.cfg_mask, return_all=return_all, cfg_drop=self.cfg_drop)
        steps = torch.linspace(1.0, 0.0, n_sampling_steps + 1, device=device)
        zs = []
        rng = range(n_sampling_steps)
        if verbose:
            try:
                from tqdm import trange
                rng = trange(n_sampling_steps, desc="sampling")
            except ImportError:
                pass
        for i in rng:
            if not noise.keyed:
                z = self.sample_zs_given_zt(zt=z, t=steps[i], s=steps[i + 1], **kwargs)
            else:                                            # a keyed chain is reproducible on this path too (not the global RNG)
                w_z, w_x, x0, scale = self.sample_zs_given_zt(zt=z, t=steps[i], s=steps[i + 1], return_ddnm=True, **kwargs)
                eps = noise.host_draw(i, z)
                z = w_z * z + w_x * x0 + scale * eps
            if return_all:
                zs.append(z)
        return torch.stack(zs, dim=0) if return_all else z


_TRAIN_GENS = {}


def train_generator(device):
    """The generator of the TRAINING step's own random draws (the stratification offset u0, the Philox seeds of the noise fields) on
    `device`: seeded once from torch.initial_seed() - identical on every rank after seed_everything(42) - and consumed by nothing
    else, so validation sampling on rank 0, user code or a rank-dependent number of draws elsewhere can never de-synchronise the
    ranks' u0 / seed sequence (the global generators are shared with all of those)."""
    key = str(torch.device(device))
    g = _TRAIN_GENS.get(key)
    if g is None:
        g = torch.Generator(device=device)
        g.manual_seed(torch.initial_seed() ^ 0x5EED)
        _TRAIN_GENS[key] = g
    return g


def reset_train_generators():
    """Forget the training generators: the next training step re-creates them from torch.initial_seed().  Call after
    torch.manual_seed / seed_everything when a run has to be reproduced inside one process (tests; entry.seed_everything does)."""
    _TRAIN_GENS.clear()


def train_generator_states():
    """{device: state} of the training generators that exist (checkpoints)."""
    return {k: g.get_state() for k, g in _TRAIN_GENS.items()}


def set_train_generator_states(states):
    """Inverse of train_generator_states(): exactly the saved generators exist afterwards, each at its saved state; any other is
    created at its first use from torch.initial_seed(), as in the run that saved them."""
    _TRAIN_GENS.clear()
    for k, st in states.items():
        g = torch.Generator(device=k)
        g.set_state(st)
        _TRAIN_GENS[k] = g


def noise_seed():
    """A fresh Philox seed for one noise field of the training step (host side; same sequence on every rank - the Philox stream id
    carries the rank)."""
    return int(torch.randint(0, 2 ** 62, (1,), generator=train_generator("cpu")).item())


def stratified_times(B, device, antithetic=True):
    """D10 antithetic sampling t_i = (u0 + i/B) mod 1, stratified over the GLOBAL batch under data parallelism: u0 comes from
    train_generator (same on all ranks) and rank r takes strata r*B .. r*B+B-1 of world*B - the variance of the t-sampling shrinks
    with the world size instead of every rank drawing the same B times."""
    rank, world = VDM._rank_world()
    g = train_generator(device)
    if antithetic:
        u0 = torch.rand(1, device=device, generator=g)
        i = torch.arange(B, device=device, dtype=torch.float32) + rank * B
        return torch.remainder(u0 + i / (world * B), 1.0)
    t = torch.rand(world * B, device=device, generator=g)
    return t[rank * B:(rank + 1) * B]


class LightVDM(nn.Module):
    """Stand-in for the LightningModule of the reference: same constructor / attributes / methods that the
    reference scripts touch; the fit loop lives in vdm4cdm_amd.trainer.Trainer."""

    def __init__(self, score_model, draw_figure=None, gamma_min=-13.3, gamma_max=13.3, noise_schedule="fixed_linear",
                 learning_rate=3.0e-4, ema_decay=None, ema_warmup=True, **vdm_kwargs):
        """ema_decay: keep an exponential moving average of the weights with this decay (ema.EmaWeights; e.g. 0.9999), updated after
        every optimizer step; None or 0: none.  ema_warmup: d_k = min(ema_decay, (1 + k) / (10 + k)) at update k."""
        super().__init__()
        from .ema import check_ema_args
        self.ema_decay, self.ema_warmup = check_ema_args(ema_decay, ema_warmup, "LightVDM(ema_decay)")      # (ValueError before any model work)
        self.ema = None                       # the EmaWeights, built by configure_optimizers (the model then sits on its device)
        self.model = VDM(score_model, noise_schedule=noise_schedule, gamma_min=gamma_min, gamma_max=gamma_max, **vdm_kwargs)
        self.draw_figure = draw_figure
        self.learning_rate = learning_rate
        self._logged = {}

    @property
    def device(self):
        return self.model.score_model.flat.device

    def log_dict(self, d):
        """Keeps the latest value per key WITHOUT reading it back (a float() here would synchronise host and GPU in every step);
        `logged` converts on access, i.e. when a logger actually wants the numbers."""
        self._logged.update({k: (v.detach() if torch.is_tensor(v) else v) for k, v in d.items()})

    @property
    def logged(self):
        return {k: float(v) for k, v in self._logged.items()}

    @staticmethod
    def _unpack(batch):
        """Batch dict contract (/root/reference/trainVDM3D128_c_c_from_field_name_thick_lowbatch.py:75-76)."""
        kw = {}
        if batch.get("conditioning") is not None:
            kw["s_conditioning"] = batch["conditioning"]
        if batch.get("conditioning_values") is not None:
            kw["v_conditionings"] = list(batch["conditioning_values"])
        return batch["x"], kw

    def _filter(self, kw):
        sm = self.model.score_model
        if not getattr(sm, "s_conditioning_channels", 1):
            kw.pop("s_conditioning", None)
        if not getattr(sm, "v_conditioning_dims", [1]):
            kw["v_conditionings"] = []
        return kw

    def training_step(self, batch, batch_idx=0):
        x, kw = self._unpack(batch)
        loss, metrics = self.model.get_loss(x, **self._filter(kw))
        self.log_dict({f"train/{k}": v for k, v in metrics.items()})
        return loss

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        x, kw = self._unpack(batch)
        loss, metrics = self.model.get_loss(x, **self._filter(kw))
        self.log_dict({f"val/{k}": v for k, v in metrics.items()})
        return loss

    def configure_optimizers(self, capturable=False):
        """capturable: the optimizer state (step count) lives on the device, so that the step can be captured in a hipGraph
        (trainer.GraphedTrainStep)."""
        fused = all(p.is_cuda for p in self.parameters())                       # one fused kernel over the flat vector
        opt = torch.optim.AdamW(self.parameters(), lr=self.learning_rate, fused=fused, capturable=bool(capturable and fused))       # D11
        sm = self.model.score_model
        from . import ema as _ema
        learned = self.model.noise_schedule == "learned_linear"
        ema = _ema.attach(self, sm, "model.score_model.",
                          {"model.gamma_b": self.model.gamma_b, "model.gamma_w": self.model.gamma_w} if learned else None)
        if hasattr(sm, "mark_weights_dirty") or ema is not None:
            def _after_step(*_):
                if hasattr(sm, "mark_weights_dirty"):      # fused steps do not bump Tensor._version: tell the HIP executor to re-pack
                    sm.mark_weights_dirty()
                    if hasattr(sm, "repack_weights"):
                        sm.repack_weights()
                if ema is not None:                        # the optimizer hook: the eager, the DDP and the captured step all average
                    ema.update()
            opt.register_step_post_hook(_after_step)
        return opt

    def ema_weights(self):
        """Context manager: inside, the model computes with the averaged weights (EmaWeights.swapped); without EMA a no-op."""
        import contextlib
        return self.ema.swapped() if self.ema is not None else contextlib.nullcontext()

    def rng_state_dict(self):
        """The random stream this module owns besides the shared training generators: the torch backend's per-rank noise generator
        (VDM._rank_noise_gen), for checkpoints."""
        g = getattr(self.model, "_noise_gen", None)
        st = {"cond_keep_calls": int(self.model._cond_keep_calls)} if self.model._cond_keep_calls else {}      # (eager conditioning dropout)
        if g is None:
            return st
        return {**st, "noise_gen": g.get_state(), "noise_gen_device": str(g.device),
                "noise_gen_key": [int(k) for k in self.model._noise_gen_key]}

    def load_rng_state_dict(self, state):
        self.model._cond_keep_calls = int(state.get("cond_keep_calls", 0))
        self.model._noise_gen = None
        if state.get("noise_gen") is not None:
            g = torch.Generator(device=state["noise_gen_device"])
            g.set_state(state["noise_gen"])
            self.model._noise_gen, self.model._noise_gen_key = g, tuple(int(k) for k in state["noise_gen_key"])

    def draw_samples(self, batch_size, n_sampling_steps=250, verbose=False, return_all=False, sampler="ancestral",
                     lower_order_final=True, **kwargs):
        """sampler: "ancestral" | "ddim" | "dpm2m" (VDM.sample)."""
        return self.model.sample(batch_size=batch_size, n_sampling_steps=n_sampling_steps, device=self.device,
                                 verbose=verbose, return_all=return_all, sampler=sampler, lower_order_final=lower_order_final, **kwargs)

    # state dict: {"model.score_model.<name>": tensor, "model.gamma_b": ..., ...}
    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = {} if destination is None else destination
        self.model.score_model.state_dict(destination=out, prefix=prefix + "model.score_model.", keep_vars=keep_vars)
        if self.model.noise_schedule == "learned_linear":
            out[prefix + "model.gamma_b"] = self.model.gamma_b.detach().clone()
            out[prefix + "model.gamma_w"] = self.model.gamma_w.detach().clone()
        return out

    def load_state_dict(self, state_dict, strict=True):
        pre = "model.score_model."
        sub = {k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}
        res = self.model.score_model.load_state_dict(sub, strict=strict)
        if self.model.noise_schedule == "learned_linear":
            with torch.no_grad():
                if "model.gamma_b" in state_dict:
                    self.model.gamma_b.copy_(state_dict["model.gamma_b"])
                if "model.gamma_w" in state_dict:
                    self.model.gamma_w.copy_(state_dict["model.gamma_w"])
        return res
