"""Minimal fit loop standing in for ``lightning.pytorch.Trainer`` on the VDM training path.

Reproduces what the reference's ``train()`` configures (/root/reference/trainVDM3D128_c_c_from_field_name_thick_lowbatch.py:28-50):
``max_steps``, ``val_check_interval``, ``gradient_clip_val=0.5`` (global L2 norm), a checkpoint every
``every_n_train_steps`` (``{"state_dict": ...}`` - the key the reference reloads, src/utils.py:468-469), an LR / metric log
(JSONL instead of Comet: no network).  Data parallelism is a build-side addition: one process per GPU,
identical weights, ONE all-reduce per step of the flat gradient vector over RCCL (``backend="nccl"`` on ROCm) or gloo on CPU.
"""
import json
import os
import sys
import time

import torch
import torch.distributed as dist

CKPT_FORMAT = 1          # layout of a checkpoint's "trainer_state" (everything beyond the weights that a resumed run needs)


def _accepts(fn, name, positional=0):
    """Does `fn` take a parameter called `name` (or **kwargs), or at least `positional` positional arguments (or *args)?  Decided from
    the signature - a TypeError raised INSIDE the user's method must surface, not silently switch graphing / sharding off."""
    import inspect
    try:
        ps = inspect.signature(fn).parameters.values()
    except (TypeError, ValueError):
        return False
    if any(p.kind == p.VAR_KEYWORD or p.name == name for p in ps):
        return True
    npos = sum(p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD) for p in ps)
    return positional > 0 and (npos >= positional or any(p.kind == p.VAR_POSITIONAL for p in ps))


def dist_env():
    return int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))


def init_distributed(device_type):
    """Initialise torch.distributed from the torchrun environment if WORLD_SIZE > 1."""
    rank, local_rank, world = dist_env()
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        backend = os.environ.get("VDM4CDM_DIST_BACKEND") or ("nccl" if device_type == "cuda" else "gloo")
        if device_type == "cuda":
            torch.cuda.set_device(local_device_index(local_rank))
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local_device_index(local_rank) if device_type == "cuda" else local_rank, world


def local_device_index(local_rank):
    """GPU of this rank: its LOCAL_RANK - or 0 for every rank under VDM4CDM_SHARE_GPU=1, the rehearsal mode that runs the N > 1 code
    path (shards, gradient buckets, barriers) with several ranks on ONE GPU (use VDM4CDM_DIST_BACKEND=gloo there: RCCL refuses two
    ranks on the same device)."""
    return 0 if os.environ.get("VDM4CDM_SHARE_GPU") == "1" else local_rank


def allreduce_mean_(t, world):
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        t.div_(world)
    return t


def clip_grad_norm_flat_(params, max_norm, use_hip, want_norm=True):
    """Global-norm clipping without a host sync.  Returns the (device) total norm (None with want_norm=False on the HIP path, where
    the coefficient never exists as a tensor: K10 sums the squares, vdm_clip_scale derives min(1, max_norm / (norm + 1e-6)) inside the
    scaling pass)."""
    grads = [p.grad for p in params if p.grad is not None]
    if use_hip:
        from . import hip_ops as ops
        acc = torch.zeros(1, device=grads[0].device)
        big = [g for g in grads if g.numel() >= 1024 and g.is_contiguous() and g.data_ptr() % 16 == 0 and g.dtype == torch.float32]
        small = [g for g in grads if not any(g is b for b in big)]
        for g in big:
            ops.sumsq(g, acc)                                   # K10
        for g in small:
            acc += (g.float() ** 2).sum()
        for g in big:
            ops.clip_scale_(g, acc, max_norm)
        if small:
            coef = torch.clamp(max_norm / (acc.sqrt() + 1e-6), max=1.0).reshape(())     # (0-dim: also scales the schedule scalars' grads)
            for g in small:
                g.mul_(coef.to(g.device))
        return acc.sqrt() if want_norm else None
    total = torch.sqrt(sum((g.float() ** 2).sum() for g in grads))
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    for g in grads:
        g.mul_(coef.to(g.device))
    return total


def rng_state(model, device):
    """Every host-side random stream a training or validation step can draw from, as a dict of plain values (checkpoints): torch's
    global CPU / device generators (the torch backend's dropout, validation sampling; torch.initial_seed() travels inside the CPU
    state), the training generators of vdm_model (u0, the Philox seeds), the HIP backend's dropout seed counter, and what the model
    itself owns (`model.rng_state_dict()`: the torch backend's per-rank noise generator)."""
    from . import vdm_model
    st = {"torch_cpu": torch.get_rng_state(), "train_generators": vdm_model.train_generator_states()}
    dev = torch.device(device)
    if dev.type == "cuda":
        st["torch_device"] = torch.cuda.get_rng_state(dev)
    uh = sys.modules.get(__package__ + ".unet_hip")
    if uh is not None:
        st["dropout_seed_counter"] = int(uh._seed_counter[0])
    if hasattr(model, "rng_state_dict"):
        st["model"] = model.rng_state_dict()
    return st


def set_rng_state(model, device, st):
    """Inverse of rng_state(): afterwards every stream continues where the saved run's did."""
    from . import vdm_model
    torch.set_rng_state(st["torch_cpu"])
    dev = torch.device(device)
    if dev.type == "cuda" and st.get("torch_device") is not None:
        torch.cuda.set_rng_state(st["torch_device"], dev)
    vdm_model.set_train_generator_states(st["train_generators"])
    if "dropout_seed_counter" in st:
        from . import unet_hip
        unet_hip._seed_counter[0] = int(st["dropout_seed_counter"])
    elif __package__ + ".unet_hip" in sys.modules:
        sys.modules[__package__ + ".unet_hip"]._seed_counter[0] = 0
    if hasattr(model, "load_rng_state_dict"):
        model.load_rng_state_dict(st.get("model") or {})


def batch_shapes(batch):
    """The shapes of every tensor of a batch dict (lists of tensors entry by entry, anything else as None): what a captured step is
    static in, whatever the batch's keys are ({"x", "conditioning", ...} of the VDM, {"x0", "x1", ...} of flow matching)."""
    def one(v):
        if torch.is_tensor(v):
            return tuple(v.shape)
        if isinstance(v, (list, tuple)):
            return tuple(one(a) for a in v)
        return None
    return {k: one(v) for k, v in batch.items()}


def cfg_dropout_record(model):
    """{"p_uncond", "cfg_drop"} of a LightVDM-like module (None: the model has no conditioning dropout, e.g. flow matching) - written
    into every checkpoint next to the trainer state; a resumed fit must match it and utils.get_model reads cfg_drop from it."""
    inner = getattr(model, "model", None)
    if inner is None or not hasattr(inner, "p_uncond"):
        return None
    return {"p_uncond": float(inner.p_uncond), "cfg_drop": str(inner.cfg_drop)}


def ema_record(model):
    """{"decay", "warmup"} of a module built with ema_decay= (None: it keeps no moving average of its weights) - what a resumed fit
    must find in the checkpoint; read from the constructor's values, the EmaWeights itself exists only after configure_optimizers."""
    if getattr(model, "ema_decay", None) is None:
        return None
    return {"decay": float(model.ema_decay), "warmup": bool(model.ema_warmup)}


def read_checkpoint(path, mmap=False):
    """A checkpoint file on the host (tensors on the CPU; mmap: mapped, so that reading `global_step` does not read the weights)."""
    return torch.load(path, map_location="cpu", mmap=bool(mmap), weights_only=True)


class GraphedTrainStep:
    """The whole training step - forward diffusion, UNet forward, ELBO, UNet backward, global-norm clip, fused AdamW, weight re-packing -
    captured ONCE in a hipGraph and replayed.  Why: the host needs ~25 us per C-ABI call; in the deep UNet
    levels the kernels are shorter than that, and the main queue idles ~1 ms per step waiting for launches (profiles/r03_step_timeline.txt).
    What makes the step capturable: static shapes (one configuration per run), no host sync on the path, RNG seeds that are kernel
    arguments PLUS a device-side step counter mixed in by the kernels (hip_ops.SEED_STEP: dropout masks, noise fields and the time grid
    change from replay to replay although the host seeds are baked into the graph), AdamW with capturable state.  Single process only:
    with world > 1 the step stays eager (the RCCL buckets are issued from Python).  The caller must not hold the loss tensor of an
    earlier EAGER step when it builds this object: its autograd graph keeps an AccumulateGrad node bound to the default stream alive,
    which would run inside the capture (torch warns; the capture then fails).
    Resume: the graph bakes in the host seeds drawn while it is captured, and the warm-up steps draw from the same generators.
    state_dict() returns the host random streams as they were immediately before construction plus the device counter; built with
    `state=` of an interrupted run the object first rewinds the streams to that point - the same seeds are baked, the same warm-up
    draws happen -, puts the caller's streams back afterwards and continues at the saved counter."""

    def __init__(self, model, opt, params, clip_val, batch, warmup=3, state=None):
        from . import hip_ops as ops
        assert ops.PROFILER is None, "per-launch events cannot be recorded inside a captured graph"
        assert ops.SEED_STEP is None, "another graphed step is being built / run in this process"
        self.model, self.opt, self.params, self.clip = model, opt, params, clip_val
        dev = params[0].device
        now = None
        if state is not None:
            now = rng_state(model, dev)
            set_rng_state(model, dev, state["rng"])
        self.rng_before = rng_state(model, dev)
        self.static = {k: ([t.clone() for t in v] if isinstance(v, (list, tuple)) else (None if v is None else v.clone())) for k, v in batch.items()}
        self.shapes = batch_shapes(batch)                       # a batch of other shapes (a ragged last one) is not for this graph
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        # The device counter is mixed into the seeds ONLY while this object's own step runs (hip_ops.SEED_STEP is set inside _step and
        # cleared on the way out): eager steps of the same process - a ragged last batch, validation, a later fit - keep drawing u0 and
        # their Philox seeds from the host generators and never see a stale counter.
        inner = getattr(model, "model", model)
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        # eager warm-up (allocator pools, workspaces, packed weights, optimizer state): NOT real steps - parameters, optimizer
        # moments / step count and the device counter are put back afterwards, so the first replay continues the optimizer where it
        # stood (step 1 of a fresh run).  State tensors the warm-up itself created (a fresh optimizer) are zeroed instead, so that
        # none is created inside the capture.
        keep = [p.detach().clone() for p in params]
        keep_state = {id(v): (v, v.detach().clone()) for st in opt.state.values() for v in st.values() if torch.is_tensor(v)}
        # the moving average of the weights (ema.EmaWeights, updated by the optimizer hook): its shadows and counter exist before the
        # warm-up - nothing of it is allocated inside the capture - and are put back with the parameters
        ema = getattr(model, "ema", None)
        keep_ema = None if ema is None else ema.snapshot()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._step()
            with torch.no_grad():
                for p, k in zip(params, keep):
                    p.copy_(k)
                for st in opt.state.values():
                    for v in st.values():
                        if torch.is_tensor(v) and id(v) in keep_state:
                            v.copy_(keep_state[id(v)][1])
                        elif torch.is_tensor(v):
                            v.zero_()
                self.counter.zero_()
                if ema is not None:
                    ema.restore(keep_ema)
            sm = getattr(inner, "score_model", None)
            if hasattr(sm, "mark_weights_dirty"):
                sm.mark_weights_dirty()
                if hasattr(sm, "repack_weights"):
                    sm.repack_weights()
        cur.wait_stream(side)
        torch.cuda.synchronize(dev)
        del keep, keep_state, keep_ema
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss, self.gnorm = self._step()
        self.replays = 0
        if state is not None:
            self.counter.fill_(int(state["counter"]))
            set_rng_state(model, dev, now)

    def state_dict(self):
        """What a checkpoint keeps of this object (reads the device counter: a host sync - checkpoint steps only)."""
        return {"counter": int(self.counter.item()), "rng": self.rng_before}

    def _step(self):
        from . import hip_ops as ops
        ops.SEED_STEP = self.counter                            # every seed of THIS step is (host seed, device step counter)
        try:
            loss = self.model.training_step(self.static, 0)
            self.opt.zero_grad(set_to_none=True)
            loss.backward()
            gnorm = clip_grad_norm_flat_(self.params, self.clip, True, want_norm=True) if self.clip else None
            self.opt.step()
            ops.step_inc(self.counter)
        finally:
            ops.SEED_STEP = None
        return loss, gnorm

    def __call__(self, batch):
        for k, v in batch.items():
            if isinstance(v, (list, tuple)):
                for dst, src in zip(self.static[k], v):
                    dst.copy_(src, non_blocking=True)
            elif v is not None:
                self.static[k].copy_(v, non_blocking=True)
        self.graph.replay()
        self.replays += 1
        return self.loss


class Trainer:
    def __init__(self, max_steps=1_000_000, val_check_interval=1000, gradient_clip_val=0.5, every_n_train_steps=10_000,
                 default_root_dir="./data/logs", experiment_name="run", limit_val_batches=4, log_every_n_steps=50,
                 n_val_sampling_steps=250, device=None, enable_progress=True, graph_step=None):
        self.max_steps, self.val_check_interval, self.gradient_clip_val = max_steps, val_check_interval, gradient_clip_val
        self.every_n_train_steps = every_n_train_steps
        self.root = os.path.join(default_root_dir, experiment_name)
        self.limit_val_batches, self.log_every_n_steps = limit_val_batches, log_every_n_steps
        self.n_val_sampling_steps = n_val_sampling_steps
        self.device = device
        self.enable_progress = enable_progress
        # capture the training step in a hipGraph (single-process HIP runs); None: $VDM4CDM_GRAPH_STEP (default off: measured 1.9 vs 5.2 ms
        # per step at 32^3 where the host is the limiter, but 15.0 vs 14.7 ms at 128^3 and 23.0 vs 21.7 ms at 64^3 fp32 - bench.py --graph)
        self.graph_step = (os.environ.get("VDM4CDM_GRAPH_STEP", "0") != "0") if graph_step is None else bool(graph_step)
        self.global_step = 0
        self.history = []
        self.optimizers, self.graphed_step = [], None           # set by fit: the optimizer; the GraphedTrainStep if the step was captured
        self._fit_ctx, self._resumed_from = None, None

    def _log(self, rec):
        if self._resumed_from is not None:                      # the first record of a resumed fit says where it came from
            rec = {**rec, "resumed_from": self._resumed_from}
            self._resumed_from = None
        self.history.append(rec)
        if self.rank == 0:
            os.makedirs(self.root, exist_ok=True)
            with open(os.path.join(self.root, "metrics.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")

    def _trainer_state(self, model, ctx):
        """Everything beyond the weights that continuing the run needs (the checkpoint's "trainer_state"): optimizer, host random
        streams, the data module's position, the graphed step's baked-seed record and counter.  Under world > 1 every rank enters ONE
        all_gather_object with its own small record (its random streams, its data-module state)."""
        dm, gstep = ctx["datamodule"], ctx["gstep"]
        rng = rng_state(model, ctx["device"])
        dm_state = dm.state_dict() if hasattr(dm, "state_dict") else None
        st = {"format": CKPT_FORMAT, "world": self.world, "optimizer": ctx["opt"].state_dict(), "rng": rng, "datamodule": dm_state,
              "batches_into_epoch": int(ctx["batches_into_epoch"]), "graph": None if gstep is None else gstep.state_dict()}
        if self.world > 1:
            recs = [None] * self.world
            dist.all_gather_object(recs, {"rank": self.rank, "rng": rng, "datamodule": dm_state})
            st["ranks"] = recs
        return st

    def save_checkpoint(self, model, epoch):
        """epoch=E-step=S.ckpt with the reference's keys (state_dict / global_step / epoch: what utils.get_model and generate_3D read)
        and, when called from fit, "trainer_state".  Written to a temporary file in the same directory and renamed: a job killed
        while saving leaves no truncated file under the final name."""
        ctx = self._fit_ctx
        state = None if ctx is None else self._trainer_state(model, ctx)      # (a collective under world > 1: every rank)
        if self.rank != 0:
            return None
        d = os.path.join(self.root, "checkpoints")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"epoch={epoch}-step={self.global_step}.ckpt")
        payload = {"state_dict": model.state_dict(), "global_step": self.global_step, "epoch": epoch}
        if cfg_dropout_record(model) is not None:
            payload["cfg_dropout"] = cfg_dropout_record(model)
        if getattr(model, "ema", None) is not None:          # the averaged weights under the model's own keys: a model loads them with
            ema_state = model.ema.state_dict()               # load_state_dict(ck["ema_state_dict"]) (reads the device counter: one sync)
            payload["ema_state_dict"] = ema_state.pop("shadow")
            payload["ema"] = ema_state                       # {"decay", "warmup", "num_updates"}
        if state is not None:
            payload["trainer_state"] = state
        tmp = f"{path}.{os.getpid()}.tmp"
        try:
            torch.save(payload, tmp)
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        return path

    @staticmethod
    def _read_resume(ckpt_path, datamodule):
        """Reads a checkpoint for fit(ckpt_path=) and checks, on the host and before any GPU work, that this run can continue it;
        positions the data module.  Returns (checkpoint, trainer_state, this rank's record)."""
        path = os.fspath(ckpt_path)
        if not os.path.isfile(path):
            raise ValueError(f"fit(ckpt_path={path!r}): no such file")
        ck = read_checkpoint(path)
        ts = ck.get("trainer_state") if isinstance(ck, dict) else None
        if ts is None:
            raise ValueError(f"{path} is a weights-only checkpoint (keys {sorted(ck) if isinstance(ck, dict) else type(ck).__name__}): it holds "
                             "no trainer_state - optimizer moments, random streams, data position - so a run cannot be resumed from it "
                             "(utils.get_model still loads it)")
        if ts.get("format") != CKPT_FORMAT:
            raise ValueError(f"{path}: trainer_state format {ts.get('format')!r}, this build reads format {CKPT_FORMAT}")
        rank, _, world = dist_env()
        if int(ts["world"]) != world:
            raise ValueError(f"{path} was written by a run of world size {ts['world']}, this run has world size {world}: a changed "
                             "world size is not covered by resume (the per-rank random streams and data shards would not line up)")
        rec = ts["ranks"][rank] if world > 1 else ts
        if not (hasattr(datamodule, "load_state_dict") and _accepts(datamodule.train_dataloader, "start_batch")):
            raise ValueError(f"fit(ckpt_path=): the data module {type(datamodule).__name__} has no state_dict() / load_state_dict() / "
                             "train_dataloader(start_batch=), so the run cannot continue at the batch after the last one consumed")
        if rec.get("datamodule") is None:
            raise ValueError(f"{path} holds no data-module state (it was written with a data module without state_dict())")
        datamodule.load_state_dict(rec["datamodule"])               # (ValueError if it is not the module that wrote the state)
        return ck, ts, rec

    def fit(self, model, datamodule, ckpt_path=None):
        """ckpt_path: a checkpoint written by fit - the run continues at its global_step, inside the same epoch at the batch after the
        last one consumed, bit for bit as if it had never stopped (same world size, batch size and data module)."""
        resume = None if ckpt_path is None else self._read_resume(ckpt_path, datamodule)
        if resume is not None:                                # conditioning dropout is part of the run, like its batch size
            saved, mine = resume[0].get("cfg_dropout") or {"p_uncond": 0.0, "cfg_drop": "v"}, cfg_dropout_record(model)
            if mine is not None and (float(saved["p_uncond"]) != mine["p_uncond"]
                                     or (mine["p_uncond"] > 0 and saved["cfg_drop"] != mine["cfg_drop"])):
                raise ValueError(f"{os.fspath(ckpt_path)} was written by a run with p_uncond={saved['p_uncond']} cfg_drop={saved['cfg_drop']!r}, "
                                 f"this model has p_uncond={mine['p_uncond']} cfg_drop={mine['cfg_drop']!r}: a resumed run must keep them")
            saved, mine = resume[0].get("ema"), ema_record(model)      # so is the moving average of the weights
            if (saved is None) != (mine is None) or (mine is not None and "ema_state_dict" not in resume[0]):
                raise ValueError(f"{os.fspath(ckpt_path)} " + ("holds no EMA of the weights" if mine is not None else
                                 f"holds an EMA of the weights (decay={saved['decay']})") + ", this model was built with ema_decay="
                                 f"{None if mine is None else mine['decay']}: a run with EMA continues only from a checkpoint that holds it, "
                                 "a run without EMA only from one that does not")
            if mine is not None and (float(saved["decay"]) != mine["decay"] or bool(saved["warmup"]) != mine["warmup"]):
                raise ValueError(f"{os.fspath(ckpt_path)} was written by a run with ema_decay={saved['decay']} ema_warmup={saved['warmup']}, "
                                 f"this model has ema_decay={mine['decay']} ema_warmup={mine['warmup']}: a resumed run must keep them")
        dev = self.device
        if dev is None:
            dev = "cuda" if torch.cuda.is_available() else "cpu"
        dev_type = torch.device(dev).type
        self.rank, local_rank, self.world = init_distributed(dev_type)
        if dev_type == "cuda":
            dev = f"cuda:{local_rank}"
            torch.cuda.set_device(local_rank)
        model.to(dev)
        if resume is not None:                                # through the model's own loader: the HIP executor re-packs its weights
            model.load_state_dict(resume[0]["state_dict"])
        datamodule.device = dev
        params = [p for p in model.parameters() if p.requires_grad]
        if self.world > 1:                                   # identical weights on every rank
            for p in params:
                dist.broadcast(p.data, src=0)
        sm = model.model.score_model
        if hasattr(sm, "enable_ddp") and dev_type == "cuda":     # HIP backend: bucketed all-reduce inside the backward pass
            sm.enable_ddp(self.world)
        use_hip = dev_type == "cuda" and getattr(model.model.score_model, "backend", "") == "hip"
        graphed = self.graph_step and use_hip and self.world == 1
        if graphed and hasattr(model.model, "graph_capturable"):      # (flow matching: the model says whether its step can be captured)
            graphed, why = model.model.graph_capturable()
            if not graphed and self.rank == 0:
                print(f"Trainer: {why} - the training step stays eager", flush=True)
        elif graphed:
            graphed = getattr(model.model, "noise_schedule", "") == "fixed_linear"
        if use_hip:
            from . import _experiment
            _experiment.refuse_for_training()      # timing switches of tools/ablate_step.sh skip kernels: never train with them
        if _accepts(model.configure_optimizers, "capturable"):
            opt = model.configure_optimizers(capturable=graphed)
        else:                                                # (a user model with the reference's zero-argument signature)
            if graphed and self.rank == 0:
                print("Trainer: configure_optimizers() takes no `capturable` argument - the training step stays eager", flush=True)
            opt, graphed = model.configure_optimizers(), False
        self.optimizers = [opt]
        gstep, graph_state = None, None
        epoch, t0, start_batch = 0, time.time(), 0
        if resume is not None:
            ck, ts, rec = resume
            graph_state = ts.get("graph")
            if graph_state is not None and not graphed:
                raise ValueError(f"{ckpt_path} was written by a run with the graph-captured training step: resume it with graph_step=True "
                                 "(VDM4CDM_GRAPH_STEP=1), the eager step draws its random numbers differently")
            how = [{k: g[k] for k in ("capturable", "fused", "foreach") if k in g} for g in opt.param_groups]
            opt.load_state_dict(ts["optimizer"])
            for g, h in zip(opt.param_groups, how):          # (how the step is executed belongs to this run, not to the saved state)
                g.update(h)
            if getattr(model, "ema", None) is not None:      # (configure_optimizers built it from the loaded weights; now its own state)
                model.ema.load_state_dict({**ck["ema"], "shadow": ck["ema_state_dict"]})
            set_rng_state(model, dev, rec["rng"])
            self.global_step, epoch, start_batch = int(ck["global_step"]), int(ck["epoch"]), int(ts["batches_into_epoch"])
            self._resumed_from = os.fspath(ckpt_path)
            resume = ck = ts = rec = None
        ctx = self._fit_ctx = {"opt": opt, "datamodule": datamodule, "device": dev, "gstep": None, "batches_into_epoch": 0}
        model.train()
        try:
            while self.global_step < self.max_steps:
                n_batches = start_batch                          # (a resumed epoch: the batches the interrupted run consumed count)
                if start_batch:
                    loader = datamodule.train_dataloader(self.rank, self.world, start_batch=start_batch)
                else:
                    loader = datamodule.train_dataloader(self.rank, self.world)
                start_batch = 0
                for batch in loader:
                    n_batches += 1
                    if graphed and gstep is None and (graph_state is not None or self.max_steps - self.global_step >= 8):
                        # captured at the first batch (its eager warm-up steps are undone: parameters / optimizer state restored)
                        gstep = ctx["gstep"] = GraphedTrainStep(model, opt, params, self.gradient_clip_val, batch, state=graph_state)
                    if gstep is not None and gstep.shapes == batch_shapes(batch):
                        loss, gnorm = gstep(batch), gstep.gnorm   # one hipGraph replay = the whole step
                    else:                                         # eager step (N > 1 ranks, short runs, a ragged last batch, the torch backend)
                        loss = model.training_step(batch, self.global_step)
                        opt.zero_grad(set_to_none=True)
                        loss.backward()
                        synced = getattr(sm, "grad_synced", False)     # the HIP backward already averaged the flat UNet gradient (in buckets)
                        sm.grad_synced = False
                        for p in params:                              # one collective per remaining parameter tensor (<= 2 schedule scalars)
                            if p.grad is not None and not (synced and p is getattr(sm, "flat", None)):
                                allreduce_mean_(p.grad, self.world)
                        gnorm = None
                        will_log = (self.global_step + 1) % self.log_every_n_steps == 0 or self.global_step == 0
                        if self.gradient_clip_val:
                            gnorm = clip_grad_norm_flat_(params, self.gradient_clip_val, use_hip, want_norm=will_log)
                        opt.step()
                    self.global_step += 1
                    if self.global_step % self.log_every_n_steps == 0 or self.global_step == 1:
                        rec = {"step": self.global_step, "epoch": epoch, "lr": opt.param_groups[0]["lr"], "time": time.time() - t0,
                               "loss": float(loss), **dict(model.logged)}
                        if gnorm is not None:
                            rec["grad_norm"] = float(gnorm)
                        self._log(rec)
                        if self.enable_progress and self.rank == 0:
                            print(f"step {self.global_step} loss {rec['loss']:.4f} ({rec['time']:.1f}s)", flush=True)
                    if self.val_check_interval and self.global_step % self.val_check_interval == 0:
                        self.validate(model, datamodule)
                    if self.every_n_train_steps and self.global_step % self.every_n_train_steps == 0:
                        ctx["batches_into_epoch"] = n_batches
                        self.save_checkpoint(model, epoch)
                    if self.global_step >= self.max_steps:
                        break
                if n_batches == 0:
                    raise RuntimeError("empty training dataloader")
                epoch += 1
        finally:
            self._fit_ctx = None
        self.graphed_step = gstep                                 # (None: every step of this fit ran eagerly)
        return self

    @torch.no_grad()
    def validate(self, model, datamodule):
        """Validation loss, samples and figure - computed with the averaged weights when the model keeps an EMA (model.ema_weights():
        parameters and shadows are exchanged in place and exchanged back, bit for bit, so the training that follows - a captured step
        included - is unaffected)."""
        import contextlib
        with (model.ema_weights() if hasattr(model, "ema_weights") else contextlib.nullcontext()):
            return self._validate(model, datamodule)

    def _validate(self, model, datamodule):
        model.eval()
        losses, last = [], None
        world = getattr(self, "world", 1)
        if _accepts(datamodule.val_dataloader, "rank", positional=2):      # the validation split is sharded like the training split
            loader = datamodule.val_dataloader(self.rank, world)
        else:                                                  # (a user datamodule with the reference's zero-argument signature)
            if world > 1 and self.rank == 0:
                print("Trainer: val_dataloader() takes no (rank, world): every rank evaluates the whole validation split", flush=True)
            loader = datamodule.val_dataloader()
        nseen = 0
        for i, batch in enumerate(loader):
            if i >= self.limit_val_batches:                    # (per rank: at world N the loss averages up to N * limit_val_batches batches)
                break
            nb = int(batch["x"].shape[0]) if isinstance(batch, dict) and torch.is_tensor(batch.get("x")) else 1
            losses.append(model.validation_step(batch, i).detach().float() * nb)      # sample-weighted: short / uneven last batches
            nseen += nb
            last = batch
        dev = losses[0].device if losses else torch.device("cpu")
        tot = torch.stack([torch.stack(losses).sum() if losses else torch.zeros((), device=dev),
                           torch.tensor(float(nseen), device=dev)])
        if world > 1:                                          # one collective, entered by EVERY rank (also one whose shard was empty)
            dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        rec = {"step": self.global_step, "val_loss": float(tot[0] / tot[1].clamp(min=1.0)), "val_samples": int(tot[1].item()), **dict(model.logged)}
        if last is not None and model.draw_figure is not None and self.rank == 0:
            x, kw = model._unpack(last)
            samples = model.draw_samples(batch_size=x.shape[0], n_sampling_steps=self.n_val_sampling_steps, **model._filter(kw))
            try:
                fig = model.draw_figure(last, samples)
                os.makedirs(self.root, exist_ok=True)
                fig.savefig(os.path.join(self.root, f"val_step{self.global_step}.png"))
            except Exception as e:                             # figures are diagnostics, never fatal to the fit loop
                rec["figure_error"] = repr(e)
        if world > 1:            # rank 0 drew the figure samples (n_val_sampling_steps denoise steps): the others wait HERE, explicitly,
            dist.barrier()       # not inside the first gradient all-reduce of the next training step
        self._log(rec)
        model.train()
        return rec
