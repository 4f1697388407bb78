"""Several conditioning fields (CUNet(s_conditioning_channels = K), K in 1..3), the parts that need no GPU: the argument checks of the
three C-ABI entries (vdm_pack_fields, vdm_diffuse_pack_fields, vdm_conv_in_dgrad_fields), the plan of conv_in's weight gradient at
cin = 3, 4, the A+B+C command line and config syntax, the data modules with three and four channel names, and a training run on the
torch backend."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ 1. C-ABI argument checks (host side, no launch)
def test_pack_fields_argument_errors(hip_lib):
    L = hip_lib

    def call(z=4096, cond=8192, k=2, n=1, per=64, dtype=1, out=16384):
        return L.vdm_pack_fields(z, cond, k, n, per, dtype, out, None)

    for name in ("z", "cond", "out"):
        assert call(**{name: None}) == -1 and b"NULL" in L.vdm_last_error(), name
    for k in (0, 4, -1):
        assert call(k=k) == -1 and b"out of range" in L.vdm_last_error()
    assert call(n=0) == -1 and b"bad sizes" in L.vdm_last_error()
    assert call(per=0) == -1 and b"bad sizes" in L.vdm_last_error()
    assert call(per=66) == -1 and b"multiple of 4" in L.vdm_last_error()
    assert call(dtype=7) == -1 and b"dtype" in L.vdm_last_error()
    for name in ("z", "cond", "out"):
        assert call(**{name: 4096 + 8}) == -1 and b"aligned" in L.vdm_last_error(), name


def test_diffuse_pack_fields_argument_errors(hip_lib):
    L = hip_lib
    ok = dict(x=4096, cond=8192, k=3, eps=None, step=None, alpha=4096, sigma=4096, n=2, per=64, dtype=0, z=4096, packed=8192)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vdm_diffuse_pack_fields(a["x"], a["cond"], a["k"], a["eps"], 1, 1, a["step"], a["alpha"], a["sigma"], a["n"], a["per"], a["dtype"],
                                         a["z"], a["packed"], None)

    for name in ("x", "cond", "alpha", "sigma", "packed"):
        assert call(**{name: None}) == -1 and b"NULL" in L.vdm_last_error(), name
    for k in (0, 4):
        assert call(k=k) == -1 and b"out of range" in L.vdm_last_error()
    assert call(n=0) == -1 and b"bad sizes" in L.vdm_last_error()
    assert call(per=62) == -1 and b"multiple of 4" in L.vdm_last_error()
    assert call(dtype=2) == -1 and b"dtype" in L.vdm_last_error()
    for name in ("x", "cond", "eps", "z", "packed"):
        assert call(**{name: 4096 + 4}) == -1 and b"aligned" in L.vdm_last_error(), name
    for name in ("alpha", "sigma", "step"):
        assert call(**{name: 4096 + 2}) == -1 and b"aligned" in L.vdm_last_error(), name


def test_conv_in_dgrad_fields_argument_errors(hip_lib):
    L = hip_lib
    ok = dict(dh=4096, n=1, d=8, h=8, w=8, c=32, dtype=1, pad=0, weight=4096, cin=3, dz=4096, ds=8192, n_ds=2)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vdm_conv_in_dgrad_fields(a["dh"], a["n"], a["d"], a["h"], a["w"], a["c"], a["dtype"], a["pad"], a["weight"], a["cin"], a["dz"],
                                          a["ds"], a["n_ds"], None)

    for name in ("dh", "weight", "dz"):
        assert call(**{name: None}) == -1 and b"NULL" in L.vdm_last_error(), name
    assert call(c=24) == -1 and b"out of range" in L.vdm_last_error()
    for cin in (0, 5):
        assert call(cin=cin, n_ds=0) == -1 and b"out of range" in L.vdm_last_error()
    for cin, n_ds in ((3, 1), (3, 3), (4, 2), (1, 1), (2, 2), (3, -1)):
        assert call(cin=cin, n_ds=n_ds) == -1 and b"n_ds" in L.vdm_last_error(), (cin, n_ds)
    assert call(ds=None) == -1 and b"ds is NULL" in L.vdm_last_error()
    assert call(d=0) == -1 and b"bad grid" in L.vdm_last_error()
    assert call(dtype=7) == -1 and b"dtype" in L.vdm_last_error()
    assert call(pad=5) == -1 and b"pad_mode" in L.vdm_last_error()
    assert call(dh=4104) == -1 and b"aligned" in L.vdm_last_error()
    assert call(dz=4098) == -1 and b"aligned" in L.vdm_last_error()
    assert call(ds=8194) == -1 and b"aligned" in L.vdm_last_error()
    # the single-field entry keeps its contract
    assert L.vdm_conv_in_dgrad(4096, 1, 8, 8, 8, 32, 1, 0, 4096, 3, 4096, None, None) == -1 and b"out of range" in L.vdm_last_error()


@pytest.mark.parametrize("circular", [False, True], ids=["zeros", "circ"])
def test_conv_in_weight_gradient_plan_leaves_the_thin_kernel_at_cin_3_and_4(hip_lib, circular):
    """plan_wgrad sends cin > 2 to the generic weight-gradient kernel (so hip_ops.gn_tail_ok is false and the unfused tail runs); the
    single-field conv_in (cin = 2) keeps the thin-input kernel."""
    from vdm4cdm_amd import _lib
    kernels = {}
    for cin in (1, 2, 3, 4):
        d = _lib.ConvDesc(n=2, od=32, oh=32, ow=32, cin=cin, cout=32, ksize=3, stride=1, upsample=0, pad_mode=int(circular), dtype=_lib.VDM_BF16,
                          out_f32=0)
        info = _lib.WgradPlanInfo()
        assert hip_lib.vdm_conv_wgrad_plan(d, 1, 0, C.byref(info)) == 0, hip_lib.vdm_last_error()
        kernels[cin] = info.kernel
        assert info.workspace_bytes == hip_lib.vdm_conv_wgrad_workspace_bytes(d) or info.kernel == _lib.WGRAD_THIN_IN
    assert kernels[1] == kernels[2] == _lib.WGRAD_THIN_IN
    assert kernels[3] == kernels[4] == _lib.WGRAD_TAPSPLIT


def test_gate_of_the_hip_backend():
    """The gate of CUNet(backend="hip").forward, reached on the CPU before any GPU work: K = 4, several input channels and 2D raise."""
    from vdm4cdm_amd.networks import CUNet
    mk = lambda shape, K: CUNet(shape=shape, chs=[8, 16], s_conditioning_channels=K, v_conditioning_dims=[], norm_groups=4, backend="hip")
    for shape, K in (((1, 8, 8, 8), 4), ((2, 8, 8, 8), 1), ((1, 8, 8), 1)):
        with pytest.raises(NotImplementedError, match="s_conditioning_channels<=3"):
            mk(shape, K)(torch.zeros((1,) + shape), t=torch.zeros(1), s_conditioning=torch.zeros((1, K) + shape[1:]))


# ------------------------------------------------------------------------------ 2. command line and configs
def test_field_list_parsing():
    from vdm4cdm_amd import data, entry
    assert entry.parse_fields("Mstar", "Mcdm") == (["Mstar", "Mcdm"], 1)
    assert entry.parse_fields("Mstar+Mgas", "Mcdm") == (["Mstar", "Mgas", "Mcdm"], 2)
    assert entry.parse_fields("Mstar+HI+T", "Mcdm") == (["Mstar", "HI", "T", "Mcdm"], 3)
    for bad in ("A+B+C+D", "A++B", "A+A", "+A", ""):
        with pytest.raises(ValueError):
            data.split_fields(bad)
        with pytest.raises(SystemExit):
            entry.parse_fields(bad, "Mcdm")
    assert entry.parse_fields("Mcdm", "Mcdm") == (["Mcdm", "Mcdm"], 1)          # the same field in and out stays accepted
    with pytest.raises(SystemExit, match="ONE source field"):
        entry.parse_fields("Mstar+Mgas", "Mcdm", multi=False)
    assert entry.parse_fields("Mstar", "Mcdm", multi=False) == (["Mstar", "Mcdm"], 1)
    # the experiment name keeps the "+"
    assert entry.VDM3D_VARIANTS["128"][4].format(i="Mstar+Mgas", o="Mcdm", c=128) == "LH128_c_c_Mstar+Mgas_to_Mcdm_thick_lowbatch_128"


@pytest.mark.parametrize("script,args,word", [
    ("trainVDM3D128_c_c_from_field_name_thick_lowbatch.py", ["A+B+C+D", "Mcdm", "16"], "at most 3"),
    ("trainVDM3D128_c_c_from_field_name_thick_lowbatch.py", ["A++B", "Mcdm", "16"], "empty field name"),
    ("train3D_c_c_from_field_name.py", ["A+A", "Mcdm"], "repeated"),
    ("train3D_c_c_from_field_name_160.py", ["A+B+C+D", "Mcdm"], "at most 3"),
    ("trainSFM3D128_c_c_from_field_name_thick_lowbatch.py", ["Mstar+Mgas", "Mcdm", "16"], "ONE source field"),
], ids=["vdm_four", "vdm_empty", "train3d_repeated", "train3d_160_four", "sfm_list"])
def test_training_scripts_refuse_a_bad_field_list_before_any_model_work(script, args, word, tmp_path):
    env = dict(os.environ, VDM4CDM_LOG_DIR=str(tmp_path), VDM4CDM_MAX_STEPS="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and word in (r.stderr + r.stdout), r.stderr[-600:]
    assert not os.listdir(tmp_path), "a run directory was created"


def _config(**kw):
    c = dict(type="VDM", ckpt_path=None, in_field_name="Mstar+Mgas", out_field_name="Mcdm", cropsize=8, chs=[8, 16], conditioning_values=6,
             data_params=dict(dataset_name="CMD_128", stage="test", batch_size=1))
    c.update(kw)
    return c


def test_get_model_and_get_datamodule_take_a_field_list(monkeypatch):
    from vdm4cdm_amd import data, utils
    monkeypatch.delenv(data.DATA_ROOT_ENV, raising=False)
    assert utils.config_fields(_config()) == (["Mstar", "Mgas"], 2)
    assert utils.config_fields(_config(in_field_name="Mstar", conditioning_channels=1)) == (["Mstar"], 1)
    assert utils.config_fields(_config(conditioning_channels=2))[1] == 2
    for k in (1, 3):
        with pytest.raises(ValueError, match="disagrees"):
            utils.get_model(_config(conditioning_channels=k), backend="torch", load_ckpt=False)
    with pytest.raises(ValueError, match="at most 3"):
        utils.get_model(_config(in_field_name="A+B+C+D"), backend="torch", load_ckpt=False)
    vdm = utils.get_model(_config(), backend="torch", load_ckpt=False)
    sm = vdm.model.score_model
    assert sm.s_conditioning_channels == 2 and sm.view("conv_in.weight").shape == (27, 8, 3)
    with pytest.warns(UserWarning, match="SYNTHETIC"):
        dm = utils.get_datamodule(_config())
    assert dm.channel_names == ["Mstar", "Mgas", "Mcdm"]
    b = next(iter(dm.test_dataloader()))
    assert b["x"].shape == (1, 1, 8, 8, 8) and b["conditioning"].shape == (1, 2, 8, 8, 8) and len(b["conditioning_values"]) == 1
    with torch.no_grad():                                    # generation passes [1, K, ...] conditioning
        out = vdm.eval().draw_samples(batch_size=2, n_sampling_steps=2, seeds=[1, 2], s_conditioning=b["conditioning"],
                                      v_conditionings=b["conditioning_values"])
    assert out.shape == (2, 1, 8, 8, 8) and torch.isfinite(out).all()


# ------------------------------------------------------------------------------ 3. data modules
def test_synthetic_module_makes_one_field_per_conditioning_name():
    from vdm4cdm_amd import data
    mk = lambda names, rf=None: data.SyntheticAstroDataModule(cropsize=8, batch_size=2, channel_names=names, return_func=rf)
    one, two = next(iter(mk(["Mstar", "Mcdm"]).train_dataloader())), next(iter(mk(["Mstar", "Mgas", "Mcdm"]).train_dataloader()))
    assert one["conditioning"].shape == (2, 1, 8, 8, 8) and two["conditioning"].shape == (2, 2, 8, 8, 8)
    assert torch.equal(two["x"], one["x"]) and torch.equal(two["conditioning"][:, :1], one["conditioning"]), "field 0 is not today's field"
    c0, c1 = two["conditioning"][:, 0], two["conditioning"][:, 1]
    assert not torch.equal(c0, c1)
    rho = torch.nn.functional.cosine_similarity(c0.flatten(), c1.flatten(), dim=0).item()
    assert 0.3 < rho < 0.999, f"the two fields should be correlated but distinct (cosine {rho})"
    # field j = standardised relu(x - (1 - 0.5 j))
    c = torch.relu(two["x"] - 0.5)
    c = c - c.mean(dim=(2, 3, 4), keepdim=True)
    assert torch.equal(c1[:, None], c / c.std(dim=(2, 3, 4), keepdim=True).clamp(min=1e-6))
    # through a return_func: fields = [c_0, c_1, c_2, x]
    seen = []
    three = mk(["Mstar", "Mgas", "T", "Mcdm"], lambda fields, params: seen.append(len(fields)) or data.cond_return_func(3)(fields, params))
    b = next(iter(three.train_dataloader()))
    assert seen == [4] and b["conditioning"].shape == (2, 3, 8, 8, 8) and torch.equal(b["conditioning"][:, :2], two["conditioning"])
    assert torch.equal(b["x"], one["x"]) and b["conditioning_values"][0].shape == (2, 6)


def test_file_backed_module_with_three_fields_and_a_normalisation_file(tmp_path, monkeypatch):
    """write_synthetic_camels-style stacks of Mstar / Mgas / Mcdm, Mgas' constants from $VDM4CDM_NORMALIZATIONS: the module holds three
    stacks, ONE augment launch serves all channels, the return_func sees fields of length 3, and the constants of all three channels
    go into the data-module state of a checkpoint.  (The launch itself is replaced by a recorder: batches are built on a GPU.)"""
    from vdm4cdm_amd import data, hip_ops
    root = data.write_synthetic_camels(str(tmp_path / "root"), dataset_name="CMD_128", n_sims=3, fullsize=8, seed=1)
    star = np.load(data.field_path(root, "CMD_128", "Astrid", "LH", "z_0.0", "Mstar"))
    np.save(data.field_path(root, "CMD_128", "Astrid", "LH", "z_0.0", "Mgas"), (3.0 * star + 1.0).astype(np.float32))
    norm = tmp_path / "norm.json"
    norm.write_text(json.dumps({"Mgas_m": 0.4, "Mgas_s": 0.25}))
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, str(norm))
    seen, launches = [], []

    def return_func(fields, params):
        seen.append(len(fields))
        return data.cond_return_func(2)(fields, params)

    dm = data.get_dataset(dataset_name="CMD_128", return_func=return_func, set_name="LH", channel_names=["Mstar", "Mgas", "Mcdm"], stage="fit",
                          batch_size=2, cropsize=4, data_root=root, seed=1)
    assert isinstance(dm, data.AstroDataModule) and len(dm.fields) == 3
    assert dm.means == [data.NORMALIZATIONS["Mstar"][0], 0.4, data.NORMALIZATIONS["Mcdm"][0]] and dm.stds[1] == 0.25
    sd = dm.state_dict()
    assert len(sd["norm"]) == 3 and sd["norm"][1] == [data.ALPHAS["Mgas"], 0.4, 0.25]
    dm.load_state_dict(sd)

    def fake_augment(fields, consts, samples, crop, out=None):
        launches.append((len(fields), len(consts), len(samples)))
        return [torch.full((len(samples), 1, crop, crop, crop), float(c)) for c in range(len(fields))]

    monkeypatch.setattr(hip_ops, "augment_batch", fake_augment)
    dm._dev_fields = [torch.from_numpy(np.array(f)) for f in dm.fields]
    dm._dev_params = torch.from_numpy(dm.params)
    b = next(iter(dm.train_dataloader()))
    assert launches == [(3, 3, 2)] and seen == [3, 3]
    assert b["conditioning"].shape == (2, 2, 4, 4, 4) and b["x"].shape == (2, 1, 4, 4, 4)
    assert bool((b["conditioning"][:, 0] == 0).all() and (b["conditioning"][:, 1] == 1).all() and (b["x"] == 2).all())
    # four names: T as a third conditioning field (its constants from the file as well)
    np.save(data.field_path(root, "CMD_128", "Astrid", "LH", "z_0.0", "T"), (0.5 * star + 2.0).astype(np.float32))
    norm.write_text(json.dumps({"Mgas_m": 0.4, "Mgas_s": 0.25, "T_m": 0.5, "T_s": 0.1}))
    dm4 = data.get_dataset(dataset_name="CMD_128", return_func=data.cond_return_func(3), set_name="LH", channel_names=["Mstar", "Mgas", "T", "Mcdm"],
                           stage="fit", batch_size=2, cropsize=4, data_root=root, seed=1)
    assert len(dm4.fields) == 4 and len(dm4.state_dict()["norm"]) == 4 and dm4.means[2] == 0.5
    dm4._dev_fields = [torch.from_numpy(np.array(f)) for f in dm4.fields]
    dm4._dev_params = torch.from_numpy(dm4.params)
    del launches[:]
    b = next(iter(dm4.train_dataloader()))
    assert launches == [(4, 4, 2)] and b["conditioning"].shape == (2, 3, 4, 4, 4)
    assert bool(all((b["conditioning"][:, j] == j).all() for j in range(3)) and (b["x"] == 3).all())


# ------------------------------------------------------------------------------ 4. training on the torch backend
def test_two_training_steps_on_the_torch_backend_with_two_fields(tmp_path):
    from helpers import randomize
    from vdm4cdm_amd import data
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.trainer import Trainer
    from vdm4cdm_amd.vdm_model import LightVDM
    torch.manual_seed(0)
    net = CUNet(shape=(1, 8, 8, 8), chs=[8, 16], s_conditioning_channels=2, v_conditioning_dims=[6], norm_groups=4, backend="torch")
    vdm = LightVDM(score_model=randomize(net, 1), draw_figure=None, gamma_max=13.3, learning_rate=1e-3)
    dm = data.SyntheticAstroDataModule(cropsize=8, batch_size=2, channel_names=["Mstar", "Mgas", "Mcdm"], return_func=data.cond_return_func(2))
    before = net.flat.detach().clone()
    tr = Trainer(max_steps=2, val_check_interval=0, every_n_train_steps=2, default_root_dir=str(tmp_path), experiment_name="k2", device="cpu",
                 enable_progress=False)
    tr.fit(vdm, dm)
    assert tr.global_step == 2 and torch.isfinite(net.flat).all() and not torch.equal(net.flat.detach(), before)
    assert not torch.equal(net.view("conv_in.weight").detach()[..., 2], net.view("conv_in.weight", before)[..., 2]), "field 1 is not trained"
    ck = torch.load(os.path.join(str(tmp_path), "k2", "checkpoints", [f for f in os.listdir(tmp_path / "k2" / "checkpoints")][0]),
                    map_location="cpu", weights_only=False)
    assert ck["state_dict"]["model.score_model.conv_in.weight"].shape[-1] == 3


def test_figure_closure_uses_channel_k_for_the_target_and_the_first_conditioning_field(monkeypatch):
    """entry._figure_closure(x_channel = K): the target images are un-normalised with the constants of channel K, the conditioning image
    shows field 0 with channel 0's constants; the figure is drawn from a batch with [B, 2, ...] conditioning."""
    pytest.importorskip("matplotlib")
    from vdm4cdm_amd import data, entry
    dm = data.SyntheticAstroDataModule(cropsize=8, batch_size=2, channel_names=["Mstar", "Mgas", "Mcdm"], return_func=data.cond_return_func(2))
    b = next(iter(dm.train_dataloader()))
    calls, real = [], dm.unnorm_func

    def unnorm(x, i_channel):
        calls.append((tuple(x.shape), i_channel))
        return real(x, i_channel)
    monkeypatch.setattr(dm, "unnorm_func", unnorm)
    fig = entry._figure_closure(dm, 4, True, x_channel=2)(b, b["x"] + 0.1)
    try:
        images = [a for a in fig.axes[:3] if a.images]
        assert len(images) == 3 and all(a.images[0].get_array().shape == (8, 8) for a in images)
        first = dm.norm_func(real(b["conditioning"][0], 0)[0, :, :, :4].sum(-1), 0).numpy()
        assert np.allclose(np.asarray(fig.axes[0].images[0].get_array()), first)
    finally:
        import matplotlib.pyplot as plt
        plt.close(fig)
    # the three images: conditioning [K, D, H, W] with channel 0, the two targets [1, D, H, W] with channel K = 2
    assert calls[:3] == [((2, 8, 8, 8), 0), ((1, 8, 8, 8), 2), ((1, 8, 8, 8), 2)]
