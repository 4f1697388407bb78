"""Batched sampling without a GPU: the argument checks of vdm_ancestral_step_rows, per-chain seeds on the torch backend, and
VDM4CDM_SAMPLE_BATCH in the sampling scripts (torch backend, single process and gloo world 2).

Bitwise checks use networks whose conv_out is zero (an untrained network, or a random one with conv_out zeroed): eps_hat = 0 exactly at
any batch size, so a chain is its z_1 and its keyed noise and must not depend on the batch it is sampled in."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from helpers import randomize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [17, 1_000_020, (1 << 40) + 5]


# ------------------------------------------------------------------------------ 6. C-ABI argument checks
def test_row_keyed_update_rejects_bad_arguments_without_a_launch(hip_lib):
    dummy = C.c_void_p(0x10000)                      # never dereferenced: every call below fails its argument check first
    f = hip_lib.vdm_ancestral_step_rows
    assert f(dummy, dummy, None, 0.0, dummy, dummy, None, 2, 64, None) == -1
    assert b"seeds" in hip_lib.vdm_last_error()
    assert f(dummy, dummy, None, 0.0, dummy, dummy, dummy, 0, 64, None) == -1
    assert b"rows" in hip_lib.vdm_last_error()
    assert f(dummy, dummy, dummy, 0.5, dummy, dummy, dummy, 2, 6, None) == -1
    assert b"per_row" in hip_lib.vdm_last_error()
    assert f(dummy, dummy, None, 0.0, dummy, dummy, dummy, 2, 0, None) == -1
    assert b"per_row" in hip_lib.vdm_last_error()
    assert f(None, dummy, None, 0.0, dummy, dummy, dummy, 2, 64, None) == -1


# ------------------------------------------------------------------------------ 7. torch backend
def _net(D=8, zero_out=True, seed=1):
    from vdm4cdm_amd.networks import CUNet
    net = CUNet(shape=(1, D, D, D), chs=[8, 16], s_conditioning_channels=1, v_conditioning_dims=[6], t_conditioning=True, norm_groups=8,
                mid_attn=False, dropout_prob=0.0, conv_padding_mode="zeros", n_attention_heads=4, backend="torch")
    randomize(net, seed)
    if zero_out:
        with torch.no_grad():
            net.view("conv_out.weight").zero_()
            net.view("conv_out.bias").zero_()
    return net


def _vdm(net, w_cfg=None):
    from vdm4cdm_amd.vdm_model import LightVDM
    return LightVDM(score_model=net, draw_figure=None, gamma_max=13.3, learning_rate=3e-4, w_cfg=w_cfg).eval()


def _cond(D, rows, seed=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, 1, D, D, D, generator=g), [torch.rand(rows, 6, generator=g)]


@pytest.mark.parametrize("w_cfg", [None, 0.7], ids=["plain", "cfg"])
@pytest.mark.parametrize("cond_rows", [3, 1], ids=["per-row-conditioning", "one-row-conditioning"])
def test_torch_backend_batched_chains_equal_single_chains(w_cfg, cond_rows):
    vdm = _vdm(_net(), w_cfg)
    s, v = _cond(8, cond_rows)
    out = vdm.draw_samples(batch_size=3, n_sampling_steps=4, seeds=SEEDS, s_conditioning=s, v_conditionings=v)
    assert out.shape == (3, 1, 8, 8, 8)
    for r, sd in enumerate(SEEDS):
        k = 0 if cond_rows == 1 else r
        one = vdm.draw_samples(batch_size=1, n_sampling_steps=4, seed=sd, s_conditioning=s[k:k + 1], v_conditionings=[v[0][k:k + 1]])
        assert torch.equal(out[r:r + 1], one), f"chain {r}"
    assert not torch.equal(out[0], out[1])


@pytest.mark.parametrize("w_cfg", [None, 0.7], ids=["plain", "cfg"])
def test_torch_backend_one_seed_list_equals_seed_on_a_random_net(w_cfg):
    vdm = _vdm(_net(zero_out=False), w_cfg)
    s, v = _cond(8, 1)
    a = vdm.draw_samples(batch_size=1, n_sampling_steps=4, seeds=[SEEDS[2]], s_conditioning=s, v_conditionings=v)
    b = vdm.draw_samples(batch_size=1, n_sampling_steps=4, seed=SEEDS[2], s_conditioning=s, v_conditionings=v)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_seeds_argument_errors_on_the_torch_backend():
    vdm = _vdm(_net())
    s, v = _cond(8, 1)
    kw = dict(n_sampling_steps=2, s_conditioning=s, v_conditionings=v)
    with pytest.raises(ValueError, match="seeds"):
        vdm.draw_samples(batch_size=3, seeds=[1, 2], **kw)
    with pytest.raises(ValueError, match="seed"):
        vdm.draw_samples(batch_size=1, seeds=[1], seed=1, **kw)
    with pytest.raises(ValueError, match="noises"):
        vdm.draw_samples(batch_size=1, seeds=[1], noises=[torch.zeros(1, 1, 8, 8, 8)] * 2, **kw)


# ------------------------------------------------------------------------------ 8. sampling scripts
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gen_cfg(tmp_path):
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "configs.yaml")))
    cfgs["VDM_Mstar_Mcdm_c_c_128"].update(cropsize=8, chs=[8, 16], ckpt_path=str(tmp_path / "none.ckpt"))
    p = tmp_path / "configs.yaml"
    yaml.safe_dump(cfgs, open(p, "w"))
    return str(p)


def _run(tmp_path, fn, runtype, out, batch, world=1, check=True):
    code = ("import sys; sys.path.insert(0, %r); from vdm4cdm_amd import entry; entry.%s(['VDM_Mstar_Mcdm_c_c_128', %r, %r], configs_path=%r)"
            % (ROOT, fn, str(out), runtype, _gen_cfg(tmp_path)))
    env = dict({k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}, OMP_NUM_THREADS="2",
               VDM4CDM_BACKEND="torch", VDM4CDM_SAMPLING_STEPS="3", VDM4CDM_REP="5", VDM4CDM_SAMPLE_BATCH=str(batch))
    if world == 1:
        cmd = [sys.executable, "-c", code]
    else:
        script = tmp_path / f"gen_worker_{fn}.py"
        script.write_text(code)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if check:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def _same_files(a, b, n_files):
    names = sorted(f.name for f in a.glob("*"))
    assert len(names) == n_files and sorted(f.name for f in b.glob("*")) == names, (names, sorted(f.name for f in b.glob("*")))
    for name in names:
        x, y = np.load(a / name), np.load(b / name)
        assert x.shape == (5, 1, 8, 8, 8) and np.array_equal(x, y), name
    g = np.load(a / names[0])
    assert not np.array_equal(g[0], g[1])


@pytest.mark.parametrize("fn,runtype,n_files", [("generate_3d", "CV_12_12", 12), ("generate_3d_1p", "1P_24", 5)])
def test_sampling_scripts_write_the_same_files_for_any_sample_batch(tmp_path, fn, runtype, n_files):
    """VDM4CDM_SAMPLE_BATCH=3 (5 repetitions: batches of 3 and 2) writes the files of VDM4CDM_SAMPLE_BATCH=1 bit for bit."""
    _run(tmp_path, fn, runtype, tmp_path / "b1", 1)
    _run(tmp_path, fn, runtype, tmp_path / "b3", 3)
    _same_files(tmp_path / "b1", tmp_path / "b3", n_files)


def test_generate_3d_batched_chains_sharded_over_gloo_world2(tmp_path):
    """torchrun world 2 (gloo) x VDM4CDM_SAMPLE_BATCH=2 writes the files of one process sampling one chain at a time, bit for bit: each rank
    batches its own round-robin share of the chains, and a chain's seed is a function of its global id only."""
    _run(tmp_path, "generate_3d", "CV_12_12", tmp_path / "w1", 1)
    _run(tmp_path, "generate_3d", "CV_12_12", tmp_path / "w2", 2, world=2)
    _same_files(tmp_path / "w1", tmp_path / "w2", 12)


@pytest.mark.parametrize("value", ["0", "x", "-2", "1.5"])
def test_sample_batch_knob_rejects_non_positive_integers(tmp_path, value):
    r = _run(tmp_path, "generate_3d", "CV_12_12", tmp_path / "bad", value, check=False)
    assert r.returncode != 0 and "VDM4CDM_SAMPLE_BATCH" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "bad").exists()                    # rejected before any output (and any model or GPU work)
