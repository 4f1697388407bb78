"""Running a sampling chain: who draws which noise field from which key (``ChainNoise``), the network part of a step (``NetStep``), the
capture-and-replay loop (``StepLoop``), and the samplers built from them - the ancestral / Euler device loop ``hip_graph_sampler``, the
deterministic multistep loop ``hip_multistep_sampler`` (DDIM, DPM-Solver++(2M), Adams-Bashforth 2; ``multistep_loop`` on the torch backend)
and the DDNM sampler (``ddnm_sample``, ``hip_ddnm_sampler``).  The model itself (schedule, loss, one-step formulas, coefficient tables) is
vdm_model.VDM; the torch-backend ancestral loop stays in ``VDM.sample``.
The table of the keying rules (mode x {z_1, host draw d, device stream}) is in DESIGN.md section 4a-s.
"""
from functools import cached_property

import torch


class _NoiseFeed:
    """Supplied noise fields (tests / oracle comparisons; the product path draws them in-kernel): uploaded in blocks of <= 256 MB and
    copied device-to-device into `buf` per draw, not one pageable host-to-device copy between every two replays."""

    def __init__(self, noises, like):
        self.noises, self.like, self.n = noises, like, len(noises)
        self.buf = torch.empty_like(like)
        self.blk = max(1, min(self.n, (256 << 20) // max(1, like.numel() * like.element_size())))
        self.first, self.block = None, None

    def load(self, i):
        first = i - i % self.blk
        if first != self.first:
            self.block = torch.stack([self.noises[k].to(dtype=self.like.dtype) for k in range(first, min(self.n, first + self.blk))]).to(
                self.like.device)
            self.first = first
        self.buf.copy_(self.block[i - first])


class ChainNoise:
    """The noise of `batch` chains over `cube` on `device`, keyed by `seed` (one stream for the batch), `seeds` (one per chain: a row is
    the batch-1 chain of its seed wherever it sits), `noises` (the fields themselves) or nothing; table in DESIGN.md 4a-s.  z1_in_noises
    is the DDNM convention: noises[0] is z_1, draw d is noises[d + 1], and the three keys exclude each other; in the ancestral convention
    draw d is noises[d] and seed= may accompany noises= (it keys z_1).  n_fields: the length `noises` must have.  `who` prefixes the
    errors.  The device side (seeds_dev, feed) is made at its first use, so the random seed of an unkeyed chain is drawn after z_1."""

    def __init__(self, who, batch, cube, device, seed=None, seeds=None, noises=None, n_fields=None, z1_in_noises=False):
        if seeds is not None:
            seeds = [int(s) for s in seeds]
            if len(seeds) != batch:
                rows = f"{batch} rows of y" if z1_in_noises else f"batch_size={batch}"
                raise ValueError(f"{who}: {len(seeds)} seeds for {rows} (one seed per chain)")
        if z1_in_noises and sum(a is not None for a in (seed, seeds, noises)) > 1:
            raise ValueError(f"{who}: seed=, seeds= and noises= cannot be combined")
        if seeds is not None and (seed is not None or noises is not None):
            raise ValueError(f"{who}: seeds= cannot be combined with seed= or noises=")
        if noises is not None and n_fields is not None and len(noises) != n_fields:
            raise ValueError(f"{who}: {len(noises)} noises, the schedule draws {n_fields} fields (z_1 first)")
        self.batch, self.cube, self.device = batch, tuple(cube), device
        self.seed, self.seeds, self.noises = None if seed is None else int(seed), seeds, noises
        self.off = 1 if z1_in_noises else 0                  # index of draw 0 in `noises`
        self.keyed = seed is not None or seeds is not None or noises is not None
        self.batch_stream = seeds is None and noises is None     # device: one Philox stream over the whole batch, not one per row
        self.like, self._gens, self._drawn = None, None, 0

    def z1(self, z=None):
        """The first field, fp32 on the device.  A caller's z is cloned (the HIP loops update z in place); seeds then key the steps only."""
        if z is not None:
            z = z.clone()
        elif self.noises is not None and self.off:
            z = self.noises[0].clone()
        elif self.seeds is not None:
            z = torch.cat([torch.randn((1, *self.cube), generator=torch.Generator().manual_seed(s)) for s in self.seeds])
        elif self.seed is not None:
            z = torch.randn((self.batch, *self.cube), generator=torch.Generator().manual_seed(self.seed))
        else:
            z = torch.randn((self.batch, *self.cube), device=self.device)
        self.like = z.to(device=self.device, dtype=torch.float32).contiguous()
        return self.like

    def host_draw(self, d, like):
        """The field of draw d on the torch backend, or None for an unkeyed chain (the loop then draws from the global RNG as it always
        did).  Generator-keyed draws are consumed in order: every chain's own generator (a (1, ...) draw per row) or the batch's."""
        if self.noises is not None:
            return self.noises[d + self.off].to(like)
        if not self.keyed:
            return None
        if self._gens is None:
            self._gens = [torch.Generator().manual_seed(s + 1) for s in (self.seeds if self.seeds is not None else [self.seed])]
        assert d == self._drawn, f"draw {d} asked of generators that are at draw {self._drawn}"
        self._drawn += 1
        if self.seeds is not None:
            return torch.cat([torch.randn((1, *like.shape[1:]), generator=g) for g in self._gens]).to(like)
        return torch.randn(like.shape, generator=self._gens[0]).to(like)

    @cached_property
    def batch_seed(self):                                    # (device side from here on)
        return self.seed if self.seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item())

    @cached_property
    def seeds_dev(self):
        """int64 on the device: one seed per row, [batch_seed] for the batch stream, None with supplied fields."""
        if self.noises is not None:
            return None
        return torch.tensor(self.seeds if self.seeds is not None else [self.batch_seed], dtype=torch.int64).to(self.device)

    @cached_property
    def feed(self):                                          # the update kernels read supplied noise from feed.buf (None: they draw it)
        return None if self.noises is None else _NoiseFeed(self.noises, self.like)

    def load(self, d):                                       # before the launch that consumes draw d: its supplied field into feed.buf
        if self.feed is not None:
            self.feed.load(d + self.off)

    def prime(self):                                         # draw 0 for the warm-up step: a plain copy, not a block upload
        self.feed.buf.copy_(self.noises[self.off].to(self.like))


class NetStep:
    """The network part of a captured step.  The conditioning of every step of a loop is known up front: ONE K6 launch embeds all time
    values t_norm (one table row per grid index), one more the vector conditionings; the step itself is [cond_table_step: gather-add of
    the rows at a device-side index, copy of z into both halves of the batch-doubled buffer under w_cfg (guided + v-masked rows of one
    forward, VDM._cfg_pair), UNet forward].  s_cond: one conditioning cube serves every row.  R: rows the UNet sees, W: table width."""

    def __init__(self, net, t_norm, z, s_cond, v_conditionings, w_cfg=None, mask_fn=None, cfg_drop="v"):
        """cfg_drop (under w_cfg): what the unguided half of the rows masks - "v": the vector conditionings (mask_fn), "s": the conditioning
        cube (zero planes, concatenated once here like s_cond itself), "vs": both."""
        from . import hip_ops as ops
        dev, B, cfg = net.flat.device, z.shape[0], w_cfg is not None
        self.net, self.B, self.W, self.R = net, B, net.table_width, 2 * B if cfg else B
        self.table_t = self.table_v = None
        with torch.no_grad():
            fl = net.flat.detach()
            if net.t_conditioning:
                self.table_t = ops.CondTable(net.cond_specs(t_norm, None, fl, which="t"), t_norm.shape[0], self.W).forward(save=False)
            vs = [v.to(device=dev, dtype=torch.float32).expand(B, -1).contiguous() for v in v_conditionings]
            if cfg:
                vs = [torch.cat([v, m], dim=0).contiguous() for v, m in zip(vs, mask_fn(vs) if "v" in cfg_drop else vs)]
            if vs:
                self.table_v = ops.CondTable(net.cond_specs(None, vs, fl, which="v"), self.R, self.W).forward(save=False)
        if s_cond is not None:
            s_cond = s_cond.to(dev).expand(B, *s_cond.shape[1:])
            s_cond = (torch.cat([s_cond, torch.zeros_like(s_cond) if "s" in cfg_drop else s_cond], dim=0) if cfg else s_cond).contiguous()
        self.s_cond = s_cond
        self.table = torch.zeros(self.R, self.W, device=dev)
        self.zz = torch.empty(self.R, *z.shape[1:], device=z.device) if cfg else None

    def __call__(self, z, row_ptr):
        """(eps_hat, eps_uncond or None) for z at the table row *row_ptr."""
        from . import hip_ops as ops
        from .unet_hip import hip_unet_apply
        if self.table_t is not None or self.table_v is not None:
            ops.cond_table_step(self.table_t, self.table_v, row_ptr, self.R, self.W, self.table)
        if self.zz is None:
            return hip_unet_apply(self.net, z, self.s_cond, table=self.table).contiguous(), None
        self.zz[:self.B].copy_(z)
        self.zz[self.B:].copy_(z)
        eps_hat = hip_unet_apply(self.net, self.zz, self.s_cond, table=self.table).contiguous()
        return eps_hat[:self.B], eps_hat[self.B:]


class StepLoop:
    """Replays `one_step` (launches that update z and `result` in place and bump their device counters) once per draw in `outer` - a
    list per outer step of the draw numbers of its steps.  With use_graph and more than 2 steps the step is warmed up on a side stream
    (packs weights, sizes the allocator; the feed is primed first on that stream), captured in a hipGraph and replayed; z and the
    counters (`reset`) are put back after each of the two.  return_all: `result` is copied out after every outer step."""

    def __init__(self, one_step, z, reset, noise, outer, result, use_graph, return_all):
        self.one_step, self.noise, self.outer, self.result = one_step, noise, outer, result
        self.count, self.graph = sum(len(draws) for draws in outer), None
        dev = z.device
        if use_graph and self.count > 2:
            z_keep = z.clone()

            def restore():
                z.copy_(z_keep)
                reset()
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                if noise.feed is not None:
                    noise.prime()
                one_step()
            torch.cuda.current_stream(dev).wait_stream(side)
            restore()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                one_step()
            restore()                       # capture does not execute, but keep the state explicit
        self.out = torch.empty((len(outer),) + tuple(result.shape), dtype=result.dtype, device=dev) if return_all else None

    def run(self, label, every, verbose, before=None):
        """before(i): launches ahead of outer step i's replays.  Returns `result`, or the stack of it after every outer step."""
        n, step = len(self.outer), self.one_step if self.graph is None else self.graph.replay
        for i, draws in enumerate(self.outer):
            if before is not None:
                before(i)
            for d in draws:
                self.noise.load(d)
                step()
            if self.out is not None:
                self.out[i].copy_(self.result)
            if verbose and (i % every == 0 or i == n - 1):
                print(f"{label} {i + 1}/{n}", flush=True)
        return self.result if self.out is None else self.out


def hip_graph_sampler(net, z, coef, noise, verbose, use_graph, s_cond, v_conditionings, w_cfg=None, mask_fn=None, return_all=False,
                      cfg_drop="v"):
    """The multi-step sampling loop on the HIP backend, shared by the VDM ancestral sampler and the SFM Euler integrator: per step
    [NetStep, fused update z <- ratio * (z - cs * net_out) + scale * noise (the w_cfg blend inside it: the guided estimate is never
    materialised), step counter + 1]; coef[n][4] = {ratio, cs, scale, network time} is read on the device at the row of the device-side
    step counter.  z is updated in place and returned; return_all: the stack [n, B, ...] of z after every step instead.  noise
    (ChainNoise): per-chain seeds go through vdm_ancestral_step_rows (row r draws from seeds[r]), anything else through K9's plain entry."""
    from . import hip_ops as ops
    step = torch.zeros(1, dtype=torch.int32, device=z.device)
    seeds_dev, seed = (noise.seeds_dev, None) if noise.seeds is not None else (None, noise.batch_seed)
    noise_buf = noise.feed and noise.feed.buf
    net_step = NetStep(net, coef[:, 3].contiguous(), z, s_cond, v_conditionings, w_cfg, mask_fn, cfg_drop)

    def one_step():
        eps_hat, eps_uncond = net_step(z, step)
        if seeds_dev is not None:
            ops.ancestral_step_rows(z, eps_hat, coef, step, seeds_dev, eps_uncond=eps_uncond, w_cfg=w_cfg or 0.0)
        else:
            ops.ancestral_step(z, eps_hat, noise_buf, coef, step, seed, eps_uncond=eps_uncond, w_cfg=w_cfg or 0.0)
        ops.step_inc(step)
    loop = StepLoop(one_step, z, step.zero_, noise, [[i] for i in range(coef.shape[0])], z, use_graph, return_all)
    return loop.run("sampling:", 50, verbose)


# ------------------------------------------------------------------------------------------------------------- multistep
VDM_SAMPLERS = ("ancestral", "ddim", "dpm2m")               # VDM.sample(sampler=); "ddim" is the order-1 multistep table


def check_sampler(name, who="sample"):
    if name not in VDM_SAMPLERS:
        raise ValueError(f"{who}: sampler={name!r} (one of {', '.join(VDM_SAMPLERS)})")
    return name


class _NoStepNoise:
    """What StepLoop asks of its noise source, for a deterministic sampler: no feed to prime, nothing to load per draw."""
    feed = None

    def load(self, d):
        pass


def hip_multistep_sampler(net, z, coef, verbose, use_graph, s_cond, v_conditionings, w_cfg=None, mask_fn=None, return_all=False,
                          cfg_drop="v"):
    """The deterministic multistep loop on the HIP backend (VDM: DDIM / DPM-Solver++(2M) on the data prediction, SFM: Euler /
    Adams-Bashforth 2 on the velocity): per step [NetStep, K9m: est = e_z z + e_e net_out (the w_cfg blend inside it), z <- w_z z +
    w_x est + w_p prev, prev <- est, step counter + 1]; coef[n][8] = {e_z, e_e, w_z, w_x, w_p, network time, 0, 0} is read on the device
    at the row of the device-side step counter.  One field of history (`prev`), no step noise.  z is updated in place and returned;
    return_all: the stack [n, B, ...] of z after every step instead."""
    from . import hip_ops as ops
    step = torch.zeros(1, dtype=torch.int32, device=z.device)
    # prev is never initialised: row 0 has w_p = 0 and K9m does not read prev there.  StepLoop's warm-up replay runs step 0 and leaves
    # its estimate in prev - harmless for the same reason (only z and the counter are put back).
    prev = torch.empty_like(z)
    net_step = NetStep(net, coef[:, 5].contiguous(), z, s_cond, v_conditionings, w_cfg, mask_fn, cfg_drop)

    def one_step():
        eps_hat, eps_uncond = net_step(z, step)
        ops.multistep_step(z, eps_hat, prev, coef, step, eps_uncond=eps_uncond, w_cfg=w_cfg or 0.0)
        ops.step_inc(step)
    loop = StepLoop(one_step, z, step.zero_, _NoStepNoise(), [[i] for i in range(coef.shape[0])], z, use_graph, return_all)
    return loop.run("sampling:", 50, verbose)


def multistep_loop(coef, z, net_out, return_all=False):
    """The same update as a plain Python loop in torch fp32 (torch backend, CPU tensors): coef [n, 8] as above, net_out(i, z) the
    network output at step i (the guided noise estimate / the velocity).  Returns z after the last step, or the stack of every step."""
    c = coef.to(dtype=torch.float32, device="cpu")
    prev, zs = None, []
    for i in range(c.shape[0]):
        e_z, e_e, w_z, w_x, w_p = (float(v) for v in c[i, :5])
        est = e_z * z + e_e * net_out(i, z)
        z = w_z * z + w_x * est
        if w_p != 0.0:
            z = z + w_p * prev
        prev = est
        if return_all:
            zs.append(z)
    return torch.stack(zs, dim=0) if return_all else z


# ------------------------------------------------------------------------------------------------------------------ DDNM
def ddnm_lengths(n_sampling_steps, l):
    """The time-travel length of every outer step as an integer array (an int: the same for all)."""
    import numpy as np
    if isinstance(l, (int, np.integer)):
        l = np.full(n_sampling_steps, int(l))
    l = np.asarray(l)
    if not (l.ndim == 1 and len(l) == n_sampling_steps and np.issubdtype(l.dtype, np.integer) and np.all(l >= 0)):
        raise ValueError("l must be a non-negative integer or an integer array of length n_sampling_steps")
    return l


def ddnm_schedule(n_sampling_steps, l):
    """The DDNM loop of /root/reference/src/utils.py:290-299 unrolled on the host.  Outer step i travels back L = min(l[i], i) grid
    steps (one draw) and then evaluates the network at t = steps[k], s = steps[k+1] for k = i-L .. i (one draw each).  Returns
    k / draw / outer: per evaluation, in order, the grid index, the number of its update draw and its outer step; L / travel_draw: per
    outer step; n_draws (z_1 is not counted: draw d is the d+1-th field after it)."""
    l = ddnm_lengths(n_sampling_steps, l)
    out = {"k": [], "draw": [], "outer": [], "L": [], "travel_draw": []}
    d = 0
    for i in range(n_sampling_steps):
        L = int(min(l[i], i))
        out["L"].append(L)
        out["travel_draw"].append(d)
        d += 1
        for j in range(L, -1, -1):
            out["k"].append(i - j)
            out["draw"].append(d)
            out["outer"].append(i)
            d += 1
    out["n_draws"] = d
    return out


def ddnm_sample(model, y, A, AT, operator, n, l, return_all, verbose, seed, seeds, noises, use_graph, device, kwargs, stats=None):
    """The seed- / noise-keyed DDNM sampler behind utils.get_ddnm_result's new keywords: on the HIP backend the device loop
    hip_ddnm_sampler, on the torch backend the reference-order loop with the same arguments (ChainNoise, DDNM convention: noises in
    call order, z_1 first).  The batch is y's row count.  stats: see utils.get_ddnm_result."""
    B, cube = y.shape[0], tuple(model.score_model.shape)
    sch = ddnm_schedule(n, l)
    noise = ChainNoise("get_ddnm_result", B, cube, device, seed, seeds, noises, n_fields=1 + sch["n_draws"], z1_in_noises=True)
    if operator is not None:
        operator.check((B,) + cube)
        A, AT = operator.A, operator.AT
    if A is None or AT is None:
        raise ValueError("get_ddnm_result: give A and AT, or operator=")
    z = noise.z1()
    y = y.to(device)
    with torch.no_grad():
        if model._hip(z):
            return hip_ddnm_sampler(model, z, y, A, AT, operator, n, sch, noise, use_graph, return_all, verbose, kwargs, stats)

        def draw(d):
            eps = noise.host_draw(d, z)
            return torch.randn_like(z) if eps is None else eps

        steps = torch.linspace(1.0, 0.0, n + 1, device=device)
        ATy = AT(y)
        xs, x_r, e = [], None, 0
        for i in range(n):
            L = sch["L"][i]
            z = model.sample_zt_given_zs(zs=z, t=steps[i - L], s=steps[i], noise=draw(sch["travel_draw"][i]))
            for _ in range(L + 1):
                k = sch["k"][e]
                w_z, w_x, x0, scale = model.sample_zs_given_zt(zt=z, t=steps[k], s=steps[k + 1], return_ddnm=True, **kwargs)
                x_r = ATy + x0 - AT(A(x0))
                z = w_z * z + w_x * x_r + scale * draw(sch["draw"][e])
                e += 1
            if return_all:
                xs.append(x_r)
        return torch.stack(xs, dim=0) if return_all else x_r


def hip_ddnm_sampler(model, z, y, A, AT, operator, n, sch, noise, use_graph, return_all, verbose, kwargs, stats=None):
    """DDNM on the HIP backend.  The captured inner step is [NetStep at k, DDNM kernels (+ the callables AT(A(.)) of a generic operator),
    cursor advance]; the host loop launches the travel-back kernel and replays the step L+1 times per outer step - no host
    synchronisation, no allocation after the capture.  All scalars come from device tables at the device cursor (ops.DdnmTables); noise
    (ChainNoise) is supplied or drawn in the kernels, keyed by (seeds[r], draw + 1) per row, or by (seed, draw + 1) over the whole
    batch.  A generic operator must be device-only torch ops with fixed shapes to be captured (use_graph=False runs the same kernels
    un-captured)."""
    from . import hip_ops as ops
    dev = z.device
    coef, travel = model.ddnm_tables(n, sch["L"])
    coef = coef.to(device=dev, dtype=torch.float32).contiguous()
    travel = travel.to(device=dev, dtype=torch.float32).contiguous()
    # (one pad row: the advance after the last evaluation reads it)
    sched = torch.tensor(list(zip(sch["k"] + sch["k"][-1:], sch["draw"] + sch["draw"][-1:])), dtype=torch.int32).to(dev)
    noise_buf = noise.feed and noise.feed.buf
    tables = ops.DdnmTables(coef, sched, noise.seeds_dev, batch_stream=noise.batch_stream)
    cfg = model.w_cfg is not None and not model.training
    if cfg:
        model._cfg_check(kwargs)
    w_cfg = float(model.w_cfg) if cfg else 0.0
    net_step = NetStep(model.score_model, coef[:, 5].contiguous(), z, kwargs.get("s_conditioning"),
                       list(kwargs.get("v_conditionings") or []), w_cfg if cfg else None, model.cfg_mask, model.cfg_drop)
    x_r = torch.empty_like(z)
    kind = getattr(operator, "kind", None)
    y = y.to(torch.float32)
    if kind == "mask":
        m = operator.mask.to(device=dev, dtype=torch.float32)
        rows = slice(0, 1) if (m.dim() < z.dim() or m.shape[0] == 1) else slice(None)
        m_dev = torch.broadcast_to(m, z.shape)[rows].contiguous()
        y_dev = torch.broadcast_to(y, z.shape).contiguous()
    elif kind == "blockmean":
        y_dev = y.contiguous()
    else:
        aty = torch.broadcast_to(AT(y).to(torch.float32), z.shape).contiguous()
        x0 = torch.empty_like(z)

    def one_step():
        eh, eu = net_step(z, tables.k_ptr)
        if kind == "mask":
            ops.ddnm_mask_step(z, eh, m_dev, y_dev, tables, noise_buf, x_r, eu, w_cfg)
        elif kind == "blockmean":
            ops.ddnm_blockmean_step(z, eh, y_dev, operator.factors, tables, noise_buf, x_r, eu, w_cfg)
        else:
            ops.ddnm_x0(z, eh, tables, x0, eu, w_cfg)
            ops.ddnm_update(z, x0, AT(A(x0)).contiguous(), aty, tables, noise_buf, x_r)
        tables.advance()

    def travel_back(i):
        if sch["L"][i] > 0:                                # (L == 0: a = 1, b = 0 - the draw is numbered, nothing is launched)
            noise.load(sch["travel_draw"][i])
            ops.ddnm_travel(z, tables, travel, i, sch["travel_draw"][i], noise_buf)

    outer = [list(range(t + 1, t + L + 2)) for t, L in zip(sch["travel_draw"], sch["L"])]       # the update draws follow the travel draw
    loop = StepLoop(one_step, z, tables.reset, noise, outer, x_r, use_graph, return_all)
    if stats is not None:
        stats.update(evaluations=loop.count, graph=loop.graph is not None, allocated_before=torch.cuda.memory_allocated(dev))
    out = loop.run("ddnm", 25, verbose, before=travel_back)
    if stats is not None:
        stats["allocated_after"] = torch.cuda.memory_allocated(dev)
    return out
