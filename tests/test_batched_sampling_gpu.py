"""Batched sampling on the HIP path: many chains per graph replay, each keyed by its own seed (VDM.sample(seeds=), the row-keyed
ancestral update vdm_ancestral_step_rows, VDM4CDM_SAMPLE_BATCH in generate_3D).

Bitwise checks use a network whose conv_out is zero: it returns eps_hat = 0 exactly at any batch size, so the whole chain is z_1 and
the keyed noise, and a chain sampled in a batch has to equal the same chain sampled alone bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from helpers import randomize

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SEEDS = [17, 1_000_020, (1 << 40) + 5, 123_456_789_012, 3, 2 ** 62 + 11]


def _net(D=16, chs=(16, 32), precision="fp32", zero_out=True, zero_init_std=0.05, seed=1):
    from vdm4cdm_amd.networks import CUNet
    net = CUNet(shape=(1, D, D, D), chs=list(chs), s_conditioning_channels=1, v_conditioning_dims=[6], t_conditioning=True,
                norm_groups=8, mid_attn=False, dropout_prob=0.0, conv_padding_mode="zeros", n_attention_heads=4, backend="hip",
                precision=precision)
    randomize(net, seed, zero_init_std=zero_init_std)
    if zero_out:
        with torch.no_grad():
            net.view("conv_out.weight").zero_()
            net.view("conv_out.bias").zero_()
    return net


def _vdm(net, w_cfg=None):
    from vdm4cdm_amd.vdm_model import LightVDM
    vdm = LightVDM(score_model=net, draw_figure=None, gamma_max=13.3, learning_rate=3e-4, w_cfg=w_cfg).to(DEV)
    return vdm.eval()


def _cond(D, rows, seed=4):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rows, 1, D, D, D, generator=g)
    v = torch.rand(rows, 6, generator=g)
    return s.to(DEV), [v.to(DEV)]


def _rows_and_singles(vdm, seeds, n, s, v, **kw):
    """(batched sample [B, ...], list of the single-chain samples [1, ...]); s / v: per-row conditioning (B rows) or one row."""
    B = len(seeds)
    out = vdm.draw_samples(batch_size=B, n_sampling_steps=n, seeds=seeds, s_conditioning=s, v_conditionings=v, **kw).cpu()
    singles = []
    for r, sd in enumerate(seeds):
        sr = s if s.shape[0] == 1 else s[r:r + 1]
        vr = [a if a.shape[0] == 1 else a[r:r + 1] for a in v]
        singles.append(vdm.draw_samples(batch_size=1, n_sampling_steps=n, seed=sd, s_conditioning=sr, v_conditionings=vr, **kw).cpu())
    return out, singles


# ------------------------------------------------------------------------------ 1. the kernel
def test_row_keyed_update_equals_one_seed_update_per_row():
    """vdm_ancestral_step_rows == vdm_ancestral_step(seed=seeds[r]) on every row alone, bit for bit: rows 1 / 3 / 5, rows of 16^3, 24^3
    (not a multiple of 1024) and 32^3 elements, step counters 0 and 7, plain and classifier-free-guided."""
    from vdm4cdm_amd import hip_ops as ops
    g = torch.Generator().manual_seed(0)
    coef = (0.5 + torch.rand(10, 4, generator=g)).to(DEV)
    for rows in (1, 3, 5):
        seeds = SEEDS[:rows]
        seeds_dev = torch.tensor(seeds, dtype=torch.int64, device=DEV)
        for D in (16, 24, 32):
            z0 = torch.randn(rows, 1, D, D, D, generator=g).to(DEV)
            eh = torch.randn(rows, 1, D, D, D, generator=g).to(DEV)
            eu = torch.randn(rows, 1, D, D, D, generator=g).to(DEV)
            for st in (0, 7):
                step = torch.full((1,), st, dtype=torch.int32, device=DEV)
                for cfg in (False, True):
                    z = z0.clone()
                    ops.ancestral_step_rows(z, eh, coef, step, seeds_dev, eps_uncond=eu if cfg else None, w_cfg=0.7 if cfg else 0.0)
                    for r in range(rows):
                        zr = z0[r:r + 1].clone()
                        ops.ancestral_step(zr, eh[r:r + 1].contiguous(), None, coef, step, seeds[r],
                                           eps_uncond=eu[r:r + 1].contiguous() if cfg else None, w_cfg=0.7 if cfg else 0.0)
                        assert torch.equal(z[r:r + 1], zr), f"rows={rows} D={D} step={st} cfg={cfg} row {r}"
                    assert not torch.equal(z, z0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ 2. the sampler, bitwise
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
@pytest.mark.parametrize("w_cfg", [None, 0.7], ids=["plain", "cfg"])
def test_batched_chains_equal_single_chains_on_a_zero_output_net(precision, use_graph, w_cfg):
    net = _net(precision=precision)
    vdm = _vdm(net, w_cfg)
    seeds = [SEEDS[1], SEEDS[3], SEEDS[4]]
    s, v = _cond(16, 3)
    out, singles = _rows_and_singles(vdm, seeds, 4, s, v, use_graph=use_graph)
    assert out.shape == (3, 1, 16, 16, 16) and torch.isfinite(out).all()
    for r in range(3):
        assert torch.equal(out[r:r + 1], singles[r]), f"chain {r} differs from the chain sampled alone"
    assert not torch.equal(out[0], out[1])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("w_cfg", [None, 0.7], ids=["plain", "cfg"])
def test_one_seed_list_equals_seed_on_a_random_net(precision, w_cfg):
    """seeds=[s] is the batch-1 chain of seed=s bit for bit on a random-weight network (same batch size, same plans): the row-keyed
    update with one row is the one-seed update."""
    net = _net(precision=precision, zero_out=False)
    vdm = _vdm(net, w_cfg)
    s, v = _cond(16, 1)
    for use_graph in (False, True):
        a = vdm.draw_samples(batch_size=1, n_sampling_steps=5, seeds=[SEEDS[2]], s_conditioning=s, v_conditionings=v, use_graph=use_graph)
        b = vdm.draw_samples(batch_size=1, n_sampling_steps=5, seed=SEEDS[2], s_conditioning=s, v_conditionings=v, use_graph=use_graph)
        assert torch.isfinite(a).all() and torch.equal(a, b), f"use_graph={use_graph}"
    all_a = vdm.draw_samples(batch_size=1, n_sampling_steps=4, seeds=[7], s_conditioning=s, v_conditionings=v, return_all=True)
    all_b = vdm.draw_samples(batch_size=1, n_sampling_steps=4, seed=7, s_conditioning=s, v_conditionings=v, return_all=True)
    assert all_a.shape == (4, 1, 1, 16, 16, 16) and torch.equal(all_a, all_b)


def test_seeds_argument_errors():
    vdm = _vdm(_net())
    s, v = _cond(16, 1)
    kw = dict(n_sampling_steps=3, s_conditioning=s, v_conditionings=v)
    with pytest.raises(ValueError):
        vdm.draw_samples(batch_size=2, seeds=[1], **kw)
    with pytest.raises(ValueError):
        vdm.draw_samples(batch_size=1, seeds=[1], seed=1, **kw)
    with pytest.raises(ValueError):
        vdm.draw_samples(batch_size=1, seeds=[1], noises=[torch.zeros(1, 1, 16, 16, 16)] * 3, **kw)
    # a supplied z: the seeds key the step noise only
    z = torch.randn(2, 1, 16, 16, 16, generator=torch.Generator().manual_seed(9))
    a = vdm.draw_samples(batch_size=2, seeds=[5, 6], z=z, **kw).cpu()
    b = vdm.draw_samples(batch_size=1, seeds=[6], z=z[1:], **kw).cpu()
    assert torch.equal(a[1:], b)


# ------------------------------------------------------------------------------ 3. a trained-like network: to rounding
def _pk(x):
    from vdm4cdm_amd import utils
    return utils.pk(x.double())[1]


@pytest.mark.parametrize("D", [16, 32])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_batched_chains_match_single_chains_on_a_near_identity_net(D, precision):
    """Random near-identity network (zero-init convs at std 0.01), n = 20: the conv plans may differ with the batch size, so a chain in
    a batch equals the chain alone only to rounding - fp32: max |d| <= 1e-4 max |single| per chain; bf16: P(k) within 1 % per bin."""
    net = _net(D=D, chs=(16, 32, 64), precision=precision, zero_out=False, zero_init_std=0.01)
    vdm = _vdm(net)
    s, v = _cond(D, 3, seed=5)
    out, singles = _rows_and_singles(vdm, [SEEDS[0], SEEDS[1], SEEDS[5]], 20, s, v)
    margins = []
    for r in range(3):
        one = singles[r]
        assert torch.isfinite(out[r]).all()
        if precision == "fp32":
            rel = (out[r:r + 1] - one).abs().max().item() / one.abs().max().item()
            margins.append(rel)
            assert rel <= 1e-4, f"chain {r}: max|d| / max|single| = {rel:.3e}"
        else:
            pb, ps = _pk(out[r:r + 1]), _pk(one)
            m = ps > 0
            rel = ((pb - ps).abs()[m] / ps[m]).max().item()
            margins.append(rel)
            assert rel <= 0.01, f"chain {r}: P(k) differs by {rel:.3e} in a bin"
    print(f"near-identity D={D} {precision}: per-chain margins {['%.2e' % m for m in margins]}")


# ------------------------------------------------------------------------------ 4. one conditioning cube for the whole batch
@pytest.mark.parametrize("w_cfg", [None, 0.7], ids=["plain", "cfg"])
def test_one_row_conditioning_broadcasts_to_the_batch(w_cfg):
    vdm = _vdm(_net(), w_cfg)
    s, v = _cond(16, 1, seed=8)
    out, singles = _rows_and_singles(vdm, SEEDS[:3], 4, s, v)
    for r in range(3):
        assert torch.equal(out[r:r + 1], singles[r]), f"chain {r}"
    # the same cube given once or once per row: the same samples
    rows = vdm.draw_samples(batch_size=3, n_sampling_steps=4, seeds=SEEDS[:3], s_conditioning=s.expand(3, -1, -1, -1, -1).contiguous(),
                            v_conditionings=[v[0].expand(3, -1).contiguous()]).cpu()
    assert torch.equal(rows, out)


# ------------------------------------------------------------------------------ 5. generate_3D
def test_generate_3d_files_do_not_depend_on_the_sample_batch(tmp_path):
    """generate_3D.py on a shrunk registry entry (cropsize 16, chs [16, 32], 5 steps, 5 repetitions): VDM4CDM_SAMPLE_BATCH = 1, 2 (ragged)
    and 8 (more than the repetitions) write the same gen_*.npy bit for bit."""
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "configs.yaml")))
    cfgs["VDM_Mstar_Mcdm_c_c_128"].update(cropsize=16, chs=[16, 32], ckpt_path=str(tmp_path / "none.ckpt"))
    cfg_path = tmp_path / "configs.yaml"
    yaml.safe_dump(cfgs, open(cfg_path, "w"))
    code = ("import os, sys; sys.path.insert(0, %r); from vdm4cdm_amd.entry import generate_3d\n"
            "for b in ('1', '2', '8'):\n"
            "    os.environ['VDM4CDM_SAMPLE_BATCH'] = b\n"
            "    generate_3d(['VDM_Mstar_Mcdm_c_c_128', os.path.join(%r, 'b' + b), 'CV_1_128'], configs_path=%r)\n"
            % (ROOT, str(tmp_path), str(cfg_path)))
    env = dict(os.environ, VDM4CDM_SAMPLING_STEPS="5", VDM4CDM_REP="5")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ref = sorted(f.name for f in (tmp_path / "b1").glob("gen_*.npy"))
    assert ref == ["gen_0.npy"]
    g1 = np.load(tmp_path / "b1" / "gen_0.npy")
    assert g1.shape == (5, 1, 16, 16, 16) and np.isfinite(g1).all() and not np.array_equal(g1[0], g1[1])
    for b in ("2", "8"):
        assert sorted(f.name for f in (tmp_path / f"b{b}").glob("gen_*.npy")) == ref
        assert np.array_equal(np.load(tmp_path / f"b{b}" / "gen_0.npy"), g1), f"VDM4CDM_SAMPLE_BATCH={b}"
