"""Resumable training on the CPU (torch backend): a fit stopped at step K and continued from its checkpoint by fresh objects is the
uninterrupted fit, BIT FOR BIT - parameters, every optimizer-state tensor, the logged losses - for both data modules, across an epoch
boundary, with validation passes in between, under gloo world 2 and in a fresh interpreter; what a resume refuses; the VDM4CDM_RESUME
knob; atomic saving.  Network and data: tests/_resume_worker.py (16^3, two levels, batch 2, dropout on)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

import _resume_worker as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K = 8, 3


@pytest.fixture(scope="module")
def synthetic_runs(tmp_path_factory):
    """Computed once: run A (N steps uninterrupted) and the first leg of run B (K steps, a checkpoint at K)."""
    root = tmp_path_factory.mktemp("resume_synthetic")
    a = W.run_fit(root, "a", N, 0)
    b1 = W.run_fit(root, "b", K, K)
    return {"root": root, "a": a, "b1": b1, "ckpt": W.ckpt_at(root, "b", K)}


def test_resume_is_bitwise_the_uninterrupted_run_synthetic(synthetic_runs):
    r = synthetic_runs
    ck = torch.load(r["ckpt"], map_location="cpu")
    ts = ck["trainer_state"]
    assert ck["global_step"] == K and ck["epoch"] == 0 and ts["format"] == 1 and ts["world"] == 1 and ts["batches_into_epoch"] == K
    assert ts["graph"] is None and "ranks" not in ts and set(ts["optimizer"]) == {"state", "param_groups"}
    assert {"torch_cpu", "train_generators", "model"} <= set(ts["rng"]) and "cpu" in ts["rng"]["train_generators"]
    before = open(r["root"] / "b" / "metrics.jsonl").read()
    b = W.run_fit(r["root"], "b", N, 0, ckpt_path=r["ckpt"])
    W.assert_same_run(r["a"], b, K, N)
    assert not torch.equal(r["b1"]["flat"], b["flat"])
    assert float(b["opt"]["0.step"]) == N
    # the same metrics.jsonl, appended to; the first record after the resume says where it came from
    text = open(r["root"] / "b" / "metrics.jsonl").read()
    assert text.startswith(before)
    recs = [json.loads(l) for l in text.splitlines()]
    assert [x["step"] for x in recs] == list(range(1, N + 1))
    assert [x.get("resumed_from") for x in recs] == [None] * K + [r["ckpt"]] + [None] * (N - K - 1)


@pytest.mark.parametrize("val", [0, 2], ids=["no_validation", "validation_every_2"])
def test_resume_is_bitwise_the_uninterrupted_run_file_backed(tmp_path, val):
    """AstroDataModule, 5 batches per epoch: K = 3 lands mid-epoch, N = 8 crosses the epoch boundary.  val=2: validation passes at
    steps 2 (before K), 4, 6 and 8 - they draw from the training generators and from the module's eval augmentation generator."""
    files = W.write_files(tmp_path / "camels")
    a = W.run_fit(tmp_path, "a", N, 0, val=val, dm=lambda: W.make_astro(files))
    W.run_fit(tmp_path, "b", K, K, val=val, dm=lambda: W.make_astro(files))
    b = W.run_fit(tmp_path, "b", N, 0, val=val, ckpt_path=W.ckpt_at(tmp_path, "b", K), dm=lambda: W.make_astro(files))
    W.assert_same_run(a, b, K, N)
    assert [h["epoch"] for h in b["history"] if "loss" in h] == [0, 0, 1, 1, 1]
    n_val = sum("val_loss" in h for h in b["history"])
    assert n_val == (3 if val else 0)
    # the resumed module built exactly the batches the uninterrupted one built after step K: the K skipped ones drew no augmentation
    # and launched nothing (run A: N training batches + one 1-item validation batch per pass)
    tail = [m for m in a["made"] if len(m) == 2][K:]
    assert [m for m in b["made"] if len(m) == 2] == tail and len(tail) == N - K
    assert len(b["made"]) == N - K + n_val


def test_file_backed_module_state_roundtrip(tmp_path):
    """state_dict / load_state_dict / train_dataloader(start_batch=) of the file-backed module on their own: a second module continues
    an epoch at batch k with the first one's batches and leaves the shuffle generator where the first one's is."""
    files = W.write_files(tmp_path / "camels")
    dm1, dm2 = W.make_astro(files), W.make_astro(files)
    for _ in dm1.train_dataloader():                           # epoch 0
        pass
    it = dm1.train_dataloader()
    first = [next(it) for _ in range(2)]                       # epoch 1, two batches in
    state = dm1.state_dict()
    rest1 = list(it)
    dm2.load_state_dict(state)
    rest2 = list(dm2.train_dataloader(0, 1, start_batch=2))
    assert len(first) == 2 and len(rest1) == len(rest2) == 3
    assert all(torch.equal(x["x"], y["x"]) and torch.equal(x["conditioning"], y["conditioning"]) for x, y in zip(rest1, rest2))
    assert torch.equal(dm1._gen.get_state(), dm2._gen.get_state())
    nxt1, nxt2 = next(iter(dm1.train_dataloader())), next(iter(dm2.train_dataloader()))          # epoch 2 starts alike
    assert torch.equal(nxt1["x"], nxt2["x"])
    # skipping a whole epoch yields nothing and still advances the shuffle generator
    dm3 = W.make_astro(files)
    dm3.load_state_dict(state)
    assert list(dm3.train_dataloader(start_batch=5)) == [] and dm3.made == []
    assert torch.equal(dm3._gen.get_state(), dm1.state_dict()["epoch_gen_state"])


class UserModule:
    """A user's data module: loaders only, no state_dict() - fine for a fresh fit, refused by a resume."""

    def __init__(self):
        self.inner = W.make_synthetic()

    def train_dataloader(self, rank=0, world=1):
        return self.inner.train_dataloader(rank, world)


def test_resume_refuses_what_it_cannot_continue(synthetic_runs, tmp_path, monkeypatch):
    from vdm4cdm_amd.trainer import Trainer
    r = synthetic_runs
    ck = torch.load(r["ckpt"], map_location="cpu")

    def refit(path, dm, match):
        W.fresh_process()
        vdm = W.make_model()
        vdm.to = None                                          # refused before the model is moved or anything else happens to it
        tr = Trainer(max_steps=N, default_root_dir=str(tmp_path), experiment_name="x", device="cpu", enable_progress=False)
        with pytest.raises(ValueError, match=match):
            tr.fit(vdm, dm, ckpt_path=path)

    old = tmp_path / "old.ckpt"                                # the format before this feature: weights only
    torch.save({k: ck[k] for k in ("state_dict", "global_step", "epoch")}, old)
    refit(str(old), W.make_synthetic(), "weights-only")
    w2 = tmp_path / "w2.ckpt"                                  # written by two ranks, resumed by one
    torch.save({**ck, "trainer_state": {**ck["trainer_state"], "world": 2, "ranks": [ck["trainer_state"]] * 2}}, w2)
    refit(str(w2), W.make_synthetic(), "world size 2.*world size 1")
    refit(r["ckpt"], W.make_synthetic(seed=6), "seed: saved 5, this module 6")
    refit(r["ckpt"], W.make_synthetic(n_train=10), "n_train: saved 8, this module 10")
    refit(str(tmp_path / "nothing.ckpt"), W.make_synthetic(), "no such file")

    refit(r["ckpt"], UserModule(), "UserModule has no state_dict")
    files = W.write_files(tmp_path / "camels")
    W.run_fit(tmp_path, "f", 2, 2, dm=lambda: W.make_astro(files))
    fck = W.ckpt_at(tmp_path, "f", 2)
    refit(fck, W.make_astro(files, seed=6), "seed: saved 5, this module 6")
    refit(fck, W.make_astro(W.write_files(tmp_path / "camels12", n_sims=12)), "nsamples: saved 11, this module 12")
    refit(fck, W.make_synthetic(), "AstroDataModule cannot be loaded into a SyntheticAstroDataModule")


def test_user_module_without_state_still_fits_fresh(tmp_path):
    from vdm4cdm_amd.trainer import Trainer
    W.fresh_process()
    tr = Trainer(max_steps=2, val_check_interval=0, every_n_train_steps=2, default_root_dir=str(tmp_path), experiment_name="u",
                 device="cpu", enable_progress=False)
    tr.fit(W.make_model(), UserModule())
    ck = torch.load(W.ckpt_at(tmp_path, "u", 2), map_location="cpu")
    assert tr.global_step == 2 and ck["trainer_state"]["datamodule"] is None


def _fake_ckpt(path, step, full=True):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({"state_dict": {}, "global_step": step, "epoch": 0, **({"trainer_state": {"format": 1}} if full else {})}, path)


def test_resume_knob_picks_the_highest_global_step_and_rejects_bad_values(tmp_path, monkeypatch):
    """VDM4CDM_RESUME in the training entry points: resolved and validated before the model is built (stubbed network: building it
    fails the test) and handed to Trainer.fit; "last" goes by the global_step stored in the files, not by mtime or name."""
    from vdm4cdm_amd import entry, networks, trainer
    monkeypatch.setenv("VDM4CDM_LOG_DIR", str(tmp_path))
    d = tmp_path / "LH_uc_uc_Mcdm" / "checkpoints"
    _fake_ckpt(str(d / "epoch=0-step=30.ckpt"), 30)
    _fake_ckpt(str(d / "epoch=9-step=9.ckpt"), 20)             # (names and mtimes disagree with the stored step)
    _fake_ckpt(str(d / "epoch=0-step=10.ckpt"), 10)
    os.utime(d / "epoch=0-step=30.ckpt", (1, 1))
    (d / "epoch=0-step=40.ckpt.123.tmp").write_bytes(b"half a file")
    built, fitted = [], []

    class Net:
        def __init__(self, *a, **kw):
            built.append(kw)
            raise AssertionError("the model must not be built")

    monkeypatch.setattr(networks, "CUNet", Net)
    for value, msg in [("nowhere.ckpt", "no such file"), ("", "no such file"), (str(d / "epoch=0-step=40.ckpt.123.tmp"), "not a readable")]:
        monkeypatch.setenv("VDM4CDM_RESUME", value)
        with pytest.raises(SystemExit, match="VDM4CDM_RESUME=.*" + msg):
            entry.train_uc_uc(["Mcdm"])
    _fake_ckpt(str(d / "old.ckpt"), 50, full=False)
    monkeypatch.setenv("VDM4CDM_RESUME", "last")
    with pytest.raises(SystemExit, match="VDM4CDM_RESUME='last'.*old.ckpt is a weights-only checkpoint"):
        entry.train_uc_uc(["Mcdm"])
    os.remove(d / "old.ckpt")
    monkeypatch.setenv("VDM4CDM_LOG_DIR", str(tmp_path / "empty"))
    with pytest.raises(SystemExit, match="VDM4CDM_RESUME=last: no readable checkpoint"):
        entry.train_sfm3d("128", ["Mstar", "Mcdm", "16"])
    assert not built
    # a good value reaches Trainer.fit of the VDM and the SFM entry points alike
    monkeypatch.setenv("VDM4CDM_LOG_DIR", str(tmp_path))
    monkeypatch.setattr(networks, "CUNet", lambda *a, **kw: torch.nn.Linear(1, 1))
    monkeypatch.setattr(trainer.Trainer, "fit", lambda self, model, datamodule, ckpt_path=None: fitted.append(ckpt_path))
    entry.train_uc_uc(["Mcdm"])
    _fake_ckpt(str(tmp_path / "LH_c_uc_Mstar_to_Mcdm" / "checkpoints" / "a.ckpt"), 7)
    entry.train_sfm_c_uc_2d(["Mstar", "Mcdm"])
    monkeypatch.setenv("VDM4CDM_RESUME", str(d / "epoch=0-step=10.ckpt"))
    entry.train_uc_c(["Mcdm"])
    monkeypatch.delenv("VDM4CDM_RESUME")
    entry.train_uc_uc(["Mcdm"])
    assert fitted == [str(d / "epoch=0-step=30.ckpt"), str(tmp_path / "LH_c_uc_Mstar_to_Mcdm" / "checkpoints" / "a.ckpt"),
                      str(d / "epoch=0-step=10.ckpt"), None]


def test_checkpoint_is_written_atomically(synthetic_runs, tmp_path, monkeypatch):
    from vdm4cdm_amd.trainer import Trainer
    r = synthetic_runs
    assert sorted(os.listdir(r["root"] / "b" / "checkpoints")) == [f"epoch=0-step={K}.ckpt"]          # no temporary file remains
    tr = Trainer(default_root_dir=str(tmp_path), experiment_name="s", device="cpu")
    tr.rank, tr.world, tr.global_step = 0, 1, 5
    vdm = W.make_model()
    path = tr.save_checkpoint(vdm, 0)
    assert os.listdir(tmp_path / "s" / "checkpoints") == [os.path.basename(path)]
    good = open(path, "rb").read()
    real_save = torch.save

    def dying_save(obj, f, *a, **kw):
        real_save(obj, f, *a, **kw)
        with open(f, "r+b") as fh:                             # a job killed while saving: half a file, then the error
            fh.truncate(os.path.getsize(f) // 2)
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", dying_save)
    with pytest.raises(OSError, match="disk full"):
        tr.save_checkpoint(vdm, 0)                             # same final name: the complete file of before stays, untouched
    tr.global_step = 6
    with pytest.raises(OSError, match="disk full"):
        tr.save_checkpoint(vdm, 0)                             # a new name: nothing under it
    assert os.listdir(tmp_path / "s" / "checkpoints") == [os.path.basename(path)] and open(path, "rb").read() == good


def test_get_model_loads_a_new_format_checkpoint(synthetic_runs):
    from vdm4cdm_amd import utils
    r = synthetic_runs
    cfg = {"type": "VDM", "cropsize": 16, "chs": [8, 16], "conditioning_values": 6, "conditioning_channels": 1, "ckpt_path": r["ckpt"]}
    vdm = utils.get_model(cfg, backend="torch", precision="fp32")
    assert torch.equal(vdm.model.score_model.flat.detach(), r["b1"]["flat"])
    assert torch.load(r["ckpt"], map_location="cpu", weights_only=True)["global_step"] == K          # plain data only


def test_resume_in_a_fresh_interpreter(synthetic_runs, tmp_path):
    """The second leg of run B in a child interpreter: nothing but the file crosses over (state hidden in module globals would)."""
    r = synthetic_runs
    root = tmp_path / "logs"
    env = dict({k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}, CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_resume_worker.py"), "child", r["ckpt"], str(root),
                        str(tmp_path / "out.pt"), str(N)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    b = torch.load(tmp_path / "out.pt", weights_only=False)
    W.assert_same_run(r["a"], b, K, N)
    assert b["history"][0]["resumed_from"] == r["ckpt"] and b["history"][0]["step"] == K + 1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_resume_gloo_world2(tmp_path):
    """Two ranks (gloo): N = 6, K = 3 (2 batches per rank and epoch: K is mid-epoch).  Rank 0's file holds one record per rank; both
    ranks resume bit-identical to their uninterrupted run and to each other."""
    env = dict(os.environ, OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "_resume_worker.py"), "ddp", str(tmp_path)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    ts = torch.load(W.ckpt_at(tmp_path, "b", 3), map_location="cpu")["trainer_state"]
    assert ts["world"] == 2 and [x["rank"] for x in ts["ranks"]] == [0, 1] and ts["batches_into_epoch"] == 1
    assert all({"rng", "datamodule"} <= set(x) for x in ts["ranks"])
    r0, r1 = ts["ranks"][0]["rng"], ts["ranks"][1]["rng"]
    assert not torch.equal(r0["model"]["noise_gen"], r1["model"]["noise_gen"])          # per-rank noise streams, each kept
    outs = [torch.load(tmp_path / f"rank{k}.pt", weights_only=False) for k in range(2)]
    for o in outs:
        W.assert_same_run(o["a"], o["b"], 3, 6)
    assert torch.equal(outs[0]["b"]["flat"], outs[1]["b"]["flat"]) and torch.equal(outs[0]["a"]["flat"], outs[1]["a"]["flat"])
    assert not torch.equal(W.losses(outs[0]["b"]["history"]), W.losses(outs[1]["b"]["history"]))          # (each rank on its own shard)
