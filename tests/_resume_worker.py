"""Shared by tests/test_resume_cpu.py and tests/test_resume_gpu.py: the smallest training run of the suite (16^3 cube, two levels, batch
2, dropout 0.1 ON), run uninterrupted or stopped and resumed, and what is compared between the two.

As a script it is the worker of the two out-of-process tests:
    python _resume_worker.py child <ckpt> <root> <out.pt> <max_steps>        resume in a fresh interpreter (world 1, CPU)
    torchrun ... _resume_worker.py ddp <dir>                                 gloo world 2: run A, run B stopped at K, run B resumed
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def fresh_process():
    """What a new interpreter starts from: entry._seed_everything(42) (which resets the training generators) and the HIP backend's
    dropout seed counter at zero.  Nothing else may be carried from one run to the next - only the checkpoint file."""
    from vdm4cdm_amd.entry import _seed_everything
    _seed_everything(42)
    uh = sys.modules.get("vdm4cdm_amd.unet_hip")
    if uh is not None:
        uh._seed_counter[0] = 0


def return_func(fields, params):
    return {"conditioning": fields[0], "x": fields[1], "conditioning_values": [params]}


def make_model(backend="torch", precision="fp32", schedule="fixed_linear"):
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.vdm_model import LightVDM
    net = CUNet(shape=(1, 16, 16, 16), chs=[16, 32] if backend == "hip" else [8, 16], s_conditioning_channels=1, v_conditioning_dims=[6],
                t_conditioning=True, norm_groups=8, mid_attn=False, dropout_prob=0.1, conv_padding_mode="zeros", n_attention_heads=4,
                backend=backend, precision=precision)
    net.reset_parameters(generator=torch.Generator().manual_seed(21), zero_init_std=0.05)
    return LightVDM(score_model=net, draw_figure=None, gamma_min=-13.3, gamma_max=13.3, noise_schedule=schedule, learning_rate=3e-3)


def make_synthetic(n_train=8, seed=5):
    from vdm4cdm_amd.data import SyntheticAstroDataModule
    return SyntheticAstroDataModule(cropsize=16, batch_size=2, n_train=n_train, n_val=4, seed=seed)


def write_files(root, n_sims=11):
    """11 simulations of 16^3, one crop each: 10 training items = 5 batches of 2 per epoch, 1 validation item."""
    from vdm4cdm_amd import data
    return data.write_synthetic_camels(str(root), dataset_name="CMD_128", n_sims=n_sims, fullsize=16, seed=3)


def make_astro(root, seed=5, cpu=True):
    """The file-backed module.  cpu: its one HIP launch per batch is replaced by the numpy oracle of the same augmentation (the host
    logic under test - epoch order, lazy augmentation draws, skipping - is the module's own)."""
    from vdm4cdm_amd import data
    dm = data.AstroDataModule(selection={"dataset_name": "CMD_128", "suite_name": "Astrid", "set_name": "LH", "z_name": "z_0.0"},
                              channel_names=["Mstar", "Mcdm"], return_func=return_func, stage="fit", batch_size=2, do_crop=True,
                              cropsize=16, data_root=str(root), seed=seed)
    dm.made = []                                              # (sim, ...) tuples of every batch that was really built
    if cpu:
        from oracle import augment_oracle as ao
        params = torch.from_numpy(dm.params)

        def make_batch(samples):
            dm.made.append(list(samples))
            items = []
            for sim, anchor, flips, perm in samples:
                outs = ao.augment_sample([np.asarray(f[sim])[None] for f in dm.fields], anchor, dm.crop, flips, perm, dm.alphas, dm.means,
                                         dm.stds)
                items.append(dm.return_func(fields=[torch.from_numpy(np.ascontiguousarray(o)) for o in outs], params=params[sim]))
            return dm.collate_fn(items)

        dm.make_batch = make_batch
    return dm


def run_fit(root, name, max_steps, every, device="cpu", ckpt_path=None, val=0, graph=False, model_kw=None, dm=None):
    """One fit from a "fresh process": new model, data module and Trainer objects.  Returns what the runs are compared by."""
    from vdm4cdm_amd.trainer import Trainer
    fresh_process()
    vdm = make_model(**(model_kw or {}))
    dm = make_synthetic() if dm is None else dm()
    tr = Trainer(max_steps=max_steps, val_check_interval=val, gradient_clip_val=0.5, every_n_train_steps=every, default_root_dir=str(root),
                 experiment_name=name, device=device, enable_progress=False, log_every_n_steps=1, limit_val_batches=2, graph_step=graph)
    if ckpt_path is None:
        tr.fit(vdm, dm)
    else:
        tr.fit(vdm, dm, ckpt_path=ckpt_path)
    return result_of(tr, vdm, dm)


def result_of(tr, vdm, dm):
    opt = tr.optimizers[0]
    params = [p for g in opt.param_groups for p in g["params"]]
    state = {f"{i}.{k}": v.detach().cpu().clone() for i, p in enumerate(params) for k, v in sorted(opt.state[p].items())
             if torch.is_tensor(v)}
    gs = getattr(tr, "graphed_step", None)
    return {"flat": torch.cat([p.detach().reshape(-1).cpu() for p in params]), "opt": state, "history": list(tr.history),
            "steps": tr.global_step, "replays": None if gs is None else gs.replays, "made": getattr(dm, "made", None)}


def losses(history, after=0, key="loss"):
    """The logged values of `key` of the steps after `after`, as a float64 tensor (compared with torch.equal)."""
    return torch.tensor([h[key] for h in history if key in h and h["step"] > after], dtype=torch.float64)


def assert_same_run(a, b, after, n_steps):
    """The core property: run b (stopped and resumed) is run a (uninterrupted), bit for bit."""
    assert a["steps"] == b["steps"] == n_steps
    assert torch.equal(a["flat"], b["flat"]), f"parameters differ in {(a['flat'] != b['flat']).sum().item()} of {a['flat'].numel()} values"
    assert sorted(a["opt"]) == sorted(b["opt"]) and len(a["opt"]) >= 3
    bad = [k for k in a["opt"] if not torch.equal(a["opt"][k], b["opt"][k])]
    assert not bad, f"optimizer state differs: {bad}"
    la, lb = losses(a["history"], after), losses(b["history"], after)
    assert la.numel() == n_steps - after and torch.equal(la, lb), f"logged losses after step {after}: {la.tolist()} vs {lb.tolist()}"
    va, vb = losses(a["history"], after, "val_loss"), losses(b["history"], after, "val_loss")
    assert torch.equal(va, vb), f"validation losses after step {after}: {va.tolist()} vs {vb.tolist()}"


def ckpt_at(root, name, step):
    import glob
    found = glob.glob(os.path.join(str(root), name, "checkpoints", f"epoch=*-step={step}.ckpt"))
    assert len(found) == 1, found
    return found[0]


def _child(argv):
    ckpt, root, out, max_steps = argv[0], argv[1], argv[2], int(argv[3])
    res = run_fit(root, "b", max_steps, 0, ckpt_path=ckpt)
    torch.save({k: res[k] for k in ("flat", "opt", "history", "steps")}, out)


def _ddp(argv):
    import torch.distributed as dist
    from vdm4cdm_amd.trainer import dist_env
    out, (rank, _, world) = argv[0], dist_env()
    N, K = 6, 3
    a = run_fit(out, "a", N, 0)
    run_fit(out, "b", K, K)
    dist.barrier()                                            # (rank 0 wrote the file)
    b = run_fit(out, "b", N, 0, ckpt_path=ckpt_at(out, "b", K))
    torch.save({"a": a, "b": b}, os.path.join(out, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    {"child": _child, "ddp": _ddp}[sys.argv[1]](sys.argv[2:])
