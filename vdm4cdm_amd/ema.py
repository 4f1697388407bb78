"""Exponential moving average (EMA) of the weights: what a trained diffusion / flow model is sampled from.

``EmaWeights`` keeps one fp32 shadow per trainable parameter tensor of a Light module - the network's flat vector, plus ``gamma_b`` /
``gamma_w`` under the learned-linear schedule - and a count of its updates.  After every optimizer step

    d_k = min(decay, (1 + k) / (10 + k))   (warmup; else d_k = decay)        w = 1 - d_k        shadow += w * (param - shadow)

with every operation rounded on its own in float32 (vdm_ema_update on the HIP backend, the same sequence of torch ops elsewhere), so
the two paths and a numpy float32 reference agree bit for bit.  On the HIP backend k lives on the device and is bumped by
vdm_step_inc, so the update can sit inside a captured training step; nothing here synchronises except state_dict().
"""
import contextlib
import math

import torch


def check_ema_args(decay, warmup=True, who="ema_decay"):
    """(decay, warmup) validated: decay None or 0 -> (None, warmup): no EMA.  Anything that is no number in [0, 1) is a ValueError."""
    if decay is None:
        return None, bool(warmup)
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError(f"{who}={decay!r} is not a number (a decay in [0, 1), e.g. 0.9999; None or 0: no EMA)") from None
    if not math.isfinite(d) or not 0.0 <= d < 1.0:
        raise ValueError(f"{who}={decay!r} must be a finite number in [0, 1) (e.g. 0.9999; None or 0: no EMA)")
    return (d if d > 0.0 else None), bool(warmup)


def ema_weight(decay, warmup, k):
    """w = 1 - d_k as a Python float holding the float32 value the kernel computes for update number k."""
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
    d = f32(decay)
    if warmup:
        d = torch.minimum(d, f32(1 + int(k)) / f32(10 + int(k)))
    return float(f32(1.0) - d)


class EmaWeights:
    """net: the CUNet of the module; prefix: what the module's state_dict() puts before the network's names ("model.score_model.");
    extra: {state-dict key: parameter} of the module's other trainable tensors.  The shadows start as copies of the parameters as
    they are NOW: build it once the model sits on its device and holds the weights it trains from."""

    def __init__(self, net, prefix, decay, warmup=True, extra=None):
        decay, warmup = check_ema_args(decay, warmup, "EmaWeights(decay)")
        if decay is None:
            raise ValueError("EmaWeights(decay=0): no averaging - build no EmaWeights instead")
        self.net, self.prefix, self.decay, self.warmup = net, prefix, decay, warmup
        self.keys = ["flat"] + list(extra or {})
        self.params = [net.flat] + list((extra or {}).values())
        dev = net.flat.device
        assert all(p.device == dev and p.dtype == torch.float32 for p in self.params), "EMA: fp32 parameters on one device"
        self.shadows = [p.detach().clone(memory_format=torch.contiguous_format) for p in self.params]
        self.hip = dev.type == "cuda" and getattr(net, "backend", "") == "hip"
        # HIP: an int32 on the device (read by the kernel, bumped by vdm_step_inc: capturable); elsewhere a Python int
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev) if self.hip else 0
        self._swapped = False

    # ------------------------------------------------------------------ the update
    @property
    def num_updates(self):
        """Updates so far (HIP: reads the device counter - a host sync; checkpoints and tests only)."""
        return int(self.counter.item()) if self.hip else int(self.counter)

    @torch.no_grad()
    def update(self):
        if self._swapped:
            raise RuntimeError("EmaWeights.update() inside swapped(): the parameters hold the average, there is nothing to average")
        if self.hip:
            from . import hip_ops as ops
            for s, p in zip(self.shadows, self.params):
                ops.ema_update(s, p.detach(), self.decay, self.warmup, self.counter)
            ops.step_inc(self.counter)
            return
        w = ema_weight(self.decay, self.warmup, self.counter)
        for s, p in zip(self.shadows, self.params):
            s.add_(torch.sub(p.detach(), s).mul_(w))       # rn(e + rn(w * rn(p - e))): three ops, three roundings
        self.counter += 1

    # ------------------------------------------------------------------ evaluation under the averaged weights
    @torch.no_grad()
    def _exchange(self):
        if self.hip:
            from . import hip_ops as ops
            for s, p in zip(self.shadows, self.params):
                ops.swap_(p.detach(), s)
        else:
            for s, p in zip(self.shadows, self.params):
                tmp = torch.empty_like(s).copy_(p.detach())
                p.detach().copy_(s)
                s.copy_(tmp)
        if hasattr(self.net, "mark_weights_dirty"):
            self.net.mark_weights_dirty()
            if hasattr(self.net, "repack_weights"):
                self.net.repack_weights()

    @contextlib.contextmanager
    def swapped(self):
        """Inside: the parameters hold the averaged weights (and the shadows the raw ones), exchanged IN PLACE, so every pointer a
        captured graph holds stays valid; the packed weight copies are rebuilt.  On exit everything has its earlier bits again."""
        if self._swapped:
            raise RuntimeError("EmaWeights.swapped() is not re-entrant: the parameters already hold the averaged weights")
        self._swapped = True
        self._exchange()
        try:
            yield self
        finally:
            self._exchange()
            self._swapped = False

    # ------------------------------------------------------------------ warm-up steps of a captured training step are not real steps
    @torch.no_grad()
    def snapshot(self):
        return [s.clone() for s in self.shadows], (self.counter.clone() if self.hip else int(self.counter))

    @torch.no_grad()
    def restore(self, snap):
        for s, k in zip(self.shadows, snap[0]):
            s.copy_(k)
        if self.hip:
            self.counter.copy_(snap[1])
        else:
            self.counter = int(snap[1])

    # ------------------------------------------------------------------ checkpoints
    def _named(self):
        """[(state-dict key, shadow tensor view)] under the module's own key names: the network's names through its view() of the
        shadow flat vector, the other tensors under their module keys."""
        out = [(self.prefix + name, self.net.view(name, flat=self.shadows[0])) for name in self.net.spec.items]
        return out + list(zip(self.keys[1:], self.shadows[1:]))

    def record(self):
        return {"decay": float(self.decay), "warmup": bool(self.warmup), "num_updates": self.num_updates}

    def state_dict(self):
        """{"decay", "warmup", "num_updates", "shadow"}; `shadow` has the keys of the module's state_dict(), so a model loads the
        averaged weights with load_state_dict(shadow)."""
        if self._swapped:
            raise RuntimeError("EmaWeights.state_dict() inside swapped(): the shadows hold the raw weights")
        return {**self.record(), "shadow": {k: v.detach().clone() for k, v in self._named()}}

    @torch.no_grad()
    def load_state_dict(self, state):
        if float(state["decay"]) != float(self.decay) or bool(state["warmup"]) != bool(self.warmup):
            raise ValueError(f"EMA state with decay={state['decay']} warmup={state['warmup']} loaded into one with decay={self.decay} "
                             f"warmup={self.warmup}")
        sd = state["shadow"]
        missing = [k for k, _ in self._named() if k not in sd]
        if missing:
            raise RuntimeError(f"EmaWeights.load_state_dict: missing {missing[:5]}...")
        n = len(self.prefix)
        for k, v in self._named():
            src = self.net._convert_entry(k[n:], sd[k]) if k.startswith(self.prefix) else sd[k].detach().to(torch.float32).reshape(v.shape)
            v.copy_(src)
        if self.hip:
            self.counter.fill_(int(state["num_updates"]))
        else:
            self.counter = int(state["num_updates"])


def attach(light, net, prefix, extra=None):
    """The EmaWeights of a Light module inside configure_optimizers (None: ema_decay unset).  One that already averages these very
    parameters is kept - a second fit of the same model continues its average; else the shadows start from the parameters as they are."""
    if light.ema_decay is None:
        light.ema = None
        return None
    params = [net.flat] + list((extra or {}).values())
    covered = {id(p) for p in params}
    left = [n for n, p in light.named_parameters() if p.requires_grad and id(p) not in covered]
    if left:
        raise RuntimeError(f"ema_decay: trainable parameters {left} have no EMA shadow")
    old = getattr(light, "ema", None)
    if old is not None and len(old.params) == len(params) and all(a is b for a, b in zip(old.params, params)) \
            and old.shadows[0].device == net.flat.device and (old.decay, old.warmup) == (light.ema_decay, light.ema_warmup):
        return old
    light.ema = EmaWeights(net, prefix, light.ema_decay, light.ema_warmup, extra)
    return light.ema
