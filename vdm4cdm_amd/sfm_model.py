"""``sfm_model.SFM`` / ``sfm_model.LightSFM`` - flow matching between two fields on the same CUNet.

Mirrors the interface the reference uses for ``mltools.models.sfm_model``:
* construction ``LightSFM(velocity_model=, draw_figure=, learning_rate=)``
  (/root/reference/trainSFM3D128_c_c_from_field_name_thick_lowbatch.py:124-127, trainSFM_c_uc_from_field_name.py:116-119)
* batch dict ``{"x0": source field, "x1": target field, "conditioning_values": [params] | None}`` (:71-72) - the velocity network is
  the same ``CUNet(shape, chs, s_conditioning_channels=1, v_conditioning_dims, ...)`` as the VDM's score network (:112-123)
* validation figure ``draw_figure_sfm(batch, samples)`` reads ``batch["x1"]`` / ``batch["x0"]`` (/root/reference/src/utils.py:204-207)
The model source (``mltools.models.sfm_model``) is not in the reference tree and ``utils.get_model`` returns nothing for
``type: SFM`` (/root/reference/src/utils.py:472-473), so the arithmetic is spec D14 [INFERRED], the conditional flow matching of
Lipman et al. 2023 / Tong et al. 2023 (I-CFM) on the straight path between the paired fields:

    x_t = (1 - t) x0 + t x1 + sigma eps,   t ~ U(0, 1) (antithetic over the batch),   target velocity u = x1 - x0
    loss = mean over batch and elements of (v_theta(x_t, t; s_conditioning = x0, v_conditionings) - u)^2
    sample: x <- x + v_theta(x, t_i; x0, v) / n,  t_i = i / n, starting from x = x0       (explicit Euler, n steps)

On the HIP backend the training step is two kernels around the network: ``vdm_sfm_head`` forms x_t straight into conv_in's packed input
(noise drawn in the kernel) and ``vdm_sfm_loss`` reduces the residual and writes its gradient - x_t, eps and u never exist in memory, and
the step can be captured in a hipGraph (``trainer.GraphedTrainStep``; the times then come from the device step counter).  With
``VDM4CDM_EXPERIMENT=fused_head=0``, or a cube whose voxel count is no multiple of 4, the interpolation / target are the K7 kernel
(``vdm_diffuse``: a x + b y per sample) and the loss and its gradient the K8 kernel: the same bits, launch by launch.  The Euler loop is
the same captured hipGraph as the VDM sampler (``sampling.hip_graph_sampler``) with the coefficient table {1, -1/n, 0, t_i};
``sample(order=2)`` is Adams-Bashforth 2 after an Euler first step, x <- x + (1.5 v - 0.5 v_prev) / n, on the multistep loop
(``sampling.hip_multistep_sampler``, kernel ``vdm_multistep_step``).
"""
import torch
import torch.nn as nn

from . import _experiment
from .sampling import ChainNoise, hip_graph_sampler, hip_multistep_sampler, multistep_loop
from .vdm_model import _DiffusionLossFn, stratified_times

# Fused head and loss of the HIP training step (vdm_sfm_head + vdm_sfm_loss; fused_head=0: diffuse -> (randn -> diffuse) -> diffuse ->
# pack_input -> the VDM loss kernel, A/B) - the VDM's switch, no new one
FUSED_HEAD = bool(_experiment.get("fused_head"))


class _SfmLossFn(torch.autograd.Function):
    """0.5 sum_n coef_n sum (v_hat - (x1 - x0))^2 through vdm_sfm_loss; d loss / d v_hat = coef_n (v_hat - (x1 - x0)) comes out of the
    same pass.  No gradient reaches x0 / x1."""

    @staticmethod
    def forward(ctx, v_hat, x0, x1, coef):
        from . import hip_ops as ops
        d = torch.empty_like(v_hat)
        sums = torch.zeros(x1.shape[0], device=x1.device)
        ops.sfm_loss(v_hat.contiguous(), x0, x1, coef, sums, d)
        ctx.save_for_backward(d)
        return 0.5 * (coef * sums).sum()

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return g * d, None, None, None


class SFM(nn.Module):
    def __init__(self, velocity_model, sigma=0.0, antithetic_time_sampling=True):
        super().__init__()
        self.velocity_model = velocity_model
        self.sigma = float(sigma)
        self.antithetic_time_sampling = antithetic_time_sampling

    @property
    def score_model(self):                                   # (the trainer and the DDP hook address the network under this name)
        return self.velocity_model

    def _hip(self, ref):
        return getattr(self.velocity_model, "backend", None) == "hip" and ref.is_cuda

    def velocity(self, xt, t, x0, v_conditionings=None):
        net = self.velocity_model
        kw = {}
        if getattr(net, "s_conditioning_channels", 1):
            kw["s_conditioning"] = x0
        return net(xt, t=t, v_conditionings=list(v_conditionings or []), **kw)

    def graph_capturable(self):
        """(can trainer.GraphedTrainStep capture this model's step?, the reason if not).  The captured step takes its times from
        vdm_train_scalars (the stratified grid, u0 from the device step counter); independent uniform times are drawn on the host."""
        if not self.antithetic_time_sampling:
            return False, "antithetic_time_sampling=False draws the times from a host generator"
        return True, ""

    def _fused_loss(self, ops, x0, x1, t, eps, v_conditionings):
        """The HIP step without the chain: vdm_sfm_head forms x_t straight into conv_in's packed input (x_t itself, the noise field and
        the target x1 - x0 never exist in memory), vdm_sfm_loss reduces the residual and writes d loss / d v.  Same bits as the chain."""
        from .vdm_model import VDM, noise_seed
        net = self.velocity_model
        B, numel = x1.shape[0], x1[0].numel()
        cond = 1 if getattr(net, "s_conditioning_channels", 1) else 0
        seed, sid, e = 0, 0, None
        if self.sigma > 0.0:
            if eps is None:
                seed, sid = noise_seed(), 2 * VDM._rank_world()[0] + 1                   # (drawn where the chain's ops.randn draws it)
            else:
                e = eps.to(device=x1.device, dtype=torch.float32).contiguous()
        dt = torch.bfloat16 if net.precision == "bf16" else torch.float32
        _, xin = ops.sfm_head(x0, x1, t.contiguous(), self.sigma, dt, cond=cond, eps=e, seed=seed, stream_id=sid)
        kw = {"s_conditioning": x0} if cond else {}
        # (x1 stands in for x_t: with a packed input the network reads only the shape of its first argument)
        v = net(x1, t=t, v_conditionings=list(v_conditionings or []), _packed_input=xin, **kw)
        coef = torch.full((B,), 2.0 / (B * numel), device=x1.device)                     # loss = 0.5 sum_n coef_n S_n = mean sq. error
        return _SfmLossFn.apply(v, x0, x1, coef)

    def get_loss(self, x0, x1, times=None, eps=None, v_conditionings=None):
        B, numel = x1.shape[0], x1[0].numel()
        x0, x1 = x0.to(torch.float32).contiguous(), x1.to(torch.float32).contiguous()
        hip = self._hip(x1)
        if hip:
            from . import hip_ops as ops
        if times is not None:
            t = times.to(x1.device, torch.float32)
        elif hip and self.antithetic_time_sampling and ops.SEED_STEP is not None:
            # graph-captured step (trainer.GraphedTrainStep): the VDM's stratified grid over the global batch, u0 drawn in the kernel from
            # one fixed seed and the device step counter (row 0 of vdm_train_scalars; the schedule rows are not used)
            from .vdm_model import VDM, noise_seed
            if getattr(self, "_graph_seed", None) is None:
                self._graph_seed = noise_seed()
            rank, world = VDM._rank_world()
            t = ops.train_scalars(B, x1.device, rank, world, 0.0, 1.0, 1.0, seed=self._graph_seed)[0]
        else:
            t = stratified_times(B, x1.device, self.antithetic_time_sampling)
        if hip and FUSED_HEAD and numel % 4 == 0 and x1.dim() == 5 and x0.shape == x1.shape \
                and getattr(self.velocity_model, "s_conditioning_channels", 1) <= 1:
            loss = self._fused_loss(ops, x0, x1, t, eps, v_conditionings)
        elif hip:
            one = torch.ones(B, device=x1.device)
            xt = ops.diffuse(x1, x0, t.contiguous(), (1.0 - t).contiguous())            # t x1 + (1 - t) x0
            if self.sigma > 0.0:
                if eps is None:
                    from .vdm_model import VDM, noise_seed
                    eps = ops.randn(torch.empty_like(x1), noise_seed(), 2 * VDM._rank_world()[0] + 1)     # (per-rank Philox stream)
                xt = ops.diffuse(xt, eps.contiguous(), one, self.sigma * one)
            u = ops.diffuse(x1, x0, one, -one)                                           # target velocity x1 - x0
            v = self.velocity(xt, t, x0, v_conditionings)
            coef = torch.full((B,), 2.0 / (B * numel), device=x1.device)                 # loss = 0.5 sum_n coef_n S_n = mean sq. error
            sums = torch.zeros(B, 3, device=x1.device)
            loss = _DiffusionLossFn.apply(v, u, u, u, 0.0, coef, sums)
        else:
            bc = (B,) + (1,) * (x1.dim() - 1)
            xt = (1.0 - t).view(bc) * x0 + t.view(bc) * x1
            if self.sigma > 0.0:
                xt = xt + self.sigma * (torch.randn_like(x1) if eps is None else eps)
            v = self.velocity(xt, t, x0, v_conditionings)
            loss = ((v - (x1 - x0)) ** 2).mean()
        return loss, {"loss": loss.detach()}

    @staticmethod
    def step_table(n):
        """[n, 4] = {1, -dt, 0, t_i} for hip_graph_sampler: x <- 1 * (x - (-dt) v) + 0 * noise, network time t_i = i / n."""
        t = torch.arange(n, dtype=torch.float64) / n
        return torch.stack([torch.ones(n, dtype=torch.float64), torch.full((n,), -1.0 / n, dtype=torch.float64),
                            torch.zeros(n, dtype=torch.float64), t], dim=1)

    @staticmethod
    def multistep_table(n, order=2):
        """[n, 8] = {e_z = 0, e_e = 1, w_z = 1, w_x, w_p, t_i = i / n, 0, 0} for hip_multistep_sampler (K9m; the estimate is the
        velocity itself).  Row 0, or every row with order=1, is explicit Euler (w_x = 1/n, w_p = 0); every other row Adams-Bashforth 2 on
        the uniform grid: x <- x + (1.5 v - 0.5 v_prev) / n."""
        if order not in (1, 2):
            raise ValueError(f"multistep_table: order={order!r} (1 or 2)")
        one, zero = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        ab2 = torch.arange(n) >= (1 if order == 2 else n)
        w_x = torch.where(ab2, 1.5 * one, one) / n
        w_p = torch.where(ab2, -0.5 * one, zero) / n
        return torch.stack([zero, one, one, w_x, w_p, torch.arange(n, dtype=torch.float64) / n, zero, zero], dim=1)

    @torch.no_grad()
    def sample(self, x0, n_sampling_steps, v_conditionings=None, return_all=False, verbose=False, use_graph=True, order=1):
        """order=1: explicit Euler; order=2: Adams-Bashforth 2 after an Euler first step (one field of history, no extra network
        evaluation)."""
        if order not in (1, 2):
            raise ValueError(f"sample: order={order!r} (1 or 2)")
        x0 = x0.to(torch.float32).contiguous()
        x = x0.clone()
        if order == 2:
            coef = self.multistep_table(n_sampling_steps, 2)
            if self._hip(x):
                s_cond = x0 if getattr(self.velocity_model, "s_conditioning_channels", 1) else None
                return hip_multistep_sampler(self.velocity_model, x, coef.to(device=x.device, dtype=torch.float32).contiguous(), verbose,
                                             use_graph, s_cond, list(v_conditionings or []), return_all=return_all)

            def velocity(i, xt):
                return self.velocity(xt, torch.full((xt.shape[0],), i / n_sampling_steps, device=xt.device), x0, v_conditionings)
            return multistep_loop(coef, x, velocity, return_all)
        if self._hip(x) and not return_all:
            coef = self.step_table(n_sampling_steps).to(device=x.device, dtype=torch.float32).contiguous()
            s_cond = x0 if getattr(self.velocity_model, "s_conditioning_channels", 1) else None
            noise = ChainNoise("sample", x.shape[0], x.shape[1:], x.device, seed=0)       # (scale = 0: the update adds no noise)
            return hip_graph_sampler(self.velocity_model, x, coef, noise, verbose, use_graph, s_cond, list(v_conditionings or []))
        xs = []
        for i in range(n_sampling_steps):
            t = torch.full((x.shape[0],), i / n_sampling_steps, device=x.device)
            x = x + self.velocity(x, t, x0, v_conditionings) / n_sampling_steps
            if return_all:
                xs.append(x)
        return torch.stack(xs, dim=0) if return_all else x


class LightSFM(nn.Module):
    """Stand-in for the reference's LightningModule ``sfm_model.LightSFM`` (same constructor / batch contract); the fit loop is
    vdm4cdm_amd.trainer.Trainer, as for LightVDM."""

    def __init__(self, velocity_model, draw_figure=None, learning_rate=3.0e-4, ema_decay=None, ema_warmup=True, **sfm_kwargs):
        """ema_decay / ema_warmup: the exponential moving average of the weights, as for LightVDM."""
        super().__init__()
        from .ema import check_ema_args
        self.ema_decay, self.ema_warmup = check_ema_args(ema_decay, ema_warmup, "LightSFM(ema_decay)")      # (ValueError before any model work)
        self.ema = None                       # the EmaWeights, built by configure_optimizers (the model then sits on its device)
        self.model = SFM(velocity_model, **sfm_kwargs)
        self.draw_figure = draw_figure
        self.learning_rate = learning_rate
        self._logged = {}

    @property
    def device(self):
        return self.model.velocity_model.flat.device

    def log_dict(self, d):
        self._logged.update({k: (v.detach() if torch.is_tensor(v) else v) for k, v in d.items()})

    @property
    def logged(self):
        return {k: float(v) for k, v in self._logged.items()}

    @staticmethod
    def _unpack(batch):
        """(x1, kwargs of draw_samples) - batch contract /root/reference/trainSFM3D128_c_c_from_field_name_thick_lowbatch.py:71-72."""
        kw = {"x0": batch["x0"]}
        if batch.get("conditioning_values") is not None:
            kw["v_conditionings"] = list(batch["conditioning_values"])
        return batch["x1"], kw

    def _filter(self, kw):
        if not getattr(self.model.velocity_model, "v_conditioning_dims", [1]):
            kw["v_conditionings"] = []
        return kw

    def training_step(self, batch, batch_idx=0):
        x1, kw = self._unpack(batch)
        loss, metrics = self.model.get_loss(x1=x1, **self._filter(kw))
        self.log_dict({f"train/{k}": v for k, v in metrics.items()})
        return loss

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        x1, kw = self._unpack(batch)
        loss, metrics = self.model.get_loss(x1=x1, **self._filter(kw))
        self.log_dict({f"val/{k}": v for k, v in metrics.items()})
        return loss

    def configure_optimizers(self, capturable=False):
        """capturable: the optimizer state (step count) lives on the device, so that the step can be captured in a hipGraph
        (trainer.GraphedTrainStep)."""
        fused = all(p.is_cuda for p in self.parameters())
        opt = torch.optim.AdamW(self.parameters(), lr=self.learning_rate, fused=fused, capturable=bool(capturable and fused))
        vm = self.model.velocity_model
        from . import ema as _ema
        ema = _ema.attach(self, vm, "model.velocity_model.")
        if hasattr(vm, "mark_weights_dirty") or ema is not None:
            def _after_step(*_):
                if hasattr(vm, "mark_weights_dirty"):      # fused steps do not bump Tensor._version: tell the HIP executor to re-pack
                    vm.mark_weights_dirty()
                    if hasattr(vm, "repack_weights"):
                        vm.repack_weights()
                if ema is not None:                        # the optimizer hook: the eager, the DDP and the captured step all average
                    ema.update()
            opt.register_step_post_hook(_after_step)
        return opt

    def ema_weights(self):
        """Context manager: inside, the model computes with the averaged weights (EmaWeights.swapped); without EMA a no-op."""
        import contextlib
        return self.ema.swapped() if self.ema is not None else contextlib.nullcontext()

    def draw_samples(self, x0=None, n_sampling_steps=100, batch_size=None, verbose=False, return_all=False, order=1, **kwargs):
        """Target-field samples for the source fields x0 (batch_size is implied by x0; accepted for the trainer's call).  order: 1
        (Euler) or 2 (Adams-Bashforth 2), SFM.sample."""
        assert x0 is not None, "LightSFM.draw_samples needs the source field x0"
        return self.model.sample(x0.to(self.device), n_sampling_steps, v_conditionings=kwargs.get("v_conditionings"),
                                 return_all=return_all, verbose=verbose, use_graph=kwargs.get("use_graph", True), order=order)

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = {} if destination is None else destination
        self.model.velocity_model.state_dict(destination=out, prefix=prefix + "model.velocity_model.", keep_vars=keep_vars)
        return out

    def load_state_dict(self, state_dict, strict=True):
        pre = "model.velocity_model."
        return self.model.velocity_model.load_state_dict({k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}, strict=strict)
