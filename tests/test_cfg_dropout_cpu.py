"""Conditioning dropout for classifier-free guidance training (VDM(p_uncond=, cfg_drop=)) - everything that needs no GPU: the Philox
reference of the keep draw, the argument errors of the model and of the three C-ABI entries, the torch backend's training step and
guided score, and the knobs of the training / generation scripts."""
import math

import numpy as np
import pytest
import torch

from _cfg_ref import keep_rows
from helpers import randomize

SEED = 20240611


# ------------------------------------------------------------------------------------------ the reference draw
@pytest.mark.parametrize("step", [None, 5])
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_reference_drop_share(p, step):
    """N = 4096 rows: |drop share - p| <= 4 sqrt(p (1 - p) / N), four standard deviations of the binomial share."""
    N = 4096
    keep = keep_rows(SEED, p, 0, N, step=step)
    assert keep.dtype == np.float32 and set(np.unique(keep)) <= {0.0, 1.0}
    share = 1.0 - keep.mean()
    bound = 4.0 * math.sqrt(p * (1.0 - p) / N)
    print(f"p {p} step {step}: drop share {share:.5f} (|d| {abs(share - p):.5f}, bound {bound:.5f})")
    assert abs(share - p) <= bound


def test_reference_edges_and_row_independence():
    assert keep_rows(SEED, 0.0, 0, 4096).all() and not keep_rows(SEED, 1.0, 0, 4096).any()
    assert np.array_equal(keep_rows(SEED, 0.5, 4, 4), keep_rows(SEED, 0.5, 0, 8)[4:])
    assert np.array_equal(keep_rows(SEED, 0.5, 2 ** 32 + 5, 4, step=3), keep_rows(SEED, 0.5, 2 ** 32, 9, step=3)[5:])
    assert not np.array_equal(keep_rows(SEED, 0.5, 0, 64), keep_rows(SEED, 0.5, 0, 64, step=1))      # the step re-keys the stream
    assert not np.array_equal(keep_rows(SEED, 0.5, 0, 64), keep_rows(SEED + 1, 0.5, 0, 64))


# ------------------------------------------------------------------------------------------ argument errors
def _net(K=1, vd=(6,), backend="torch"):
    from vdm4cdm_amd.networks import CUNet
    net = CUNet(shape=(1, 8, 8, 8), chs=[8, 16], s_conditioning_channels=K, v_conditioning_dims=list(vd), norm_groups=4, backend=backend)
    return randomize(net, 5)


def _vdm(net, **kw):
    from vdm4cdm_amd.vdm_model import LightVDM
    return LightVDM(score_model=net, gamma_max=13.3, **kw)


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan"), float("inf"), "half"])
def test_p_uncond_outside_the_unit_interval_is_refused(p):
    with pytest.raises(ValueError, match="p_uncond"):
        _vdm(_net(), p_uncond=p)


def test_cfg_drop_errors():
    with pytest.raises(ValueError, match="cfg_drop"):
        _vdm(_net(), p_uncond=0.1, cfg_drop="sv")
    with pytest.raises(ValueError, match="cfg_drop"):
        _vdm(_net(), cfg_drop="x")                                         # (unknown: refused although p_uncond == 0)
    for drop in ("v", "vs"):
        with pytest.raises(ValueError, match="v_conditioning_dims"):
            _vdm(_net(vd=()), p_uncond=0.1, cfg_drop=drop)
    for drop in ("s", "vs"):
        with pytest.raises(ValueError, match="s_conditioning_channels"):
            _vdm(_net(K=0), p_uncond=0.1, cfg_drop=drop)
    with pytest.raises(ValueError, match="s_conditioning_channels"):
        _vdm(_net(K=0), w_cfg=1.0, cfg_drop="s")
    m = _vdm(_net(K=0, vd=()))                                             # the defaults stay valid for every network
    assert m.model.p_uncond == 0.0 and m.model.cfg_drop == "v" and m.model.last_cond_keep is None
    assert _vdm(_net(), p_uncond=1, cfg_drop="vs").model.p_uncond == 1.0


def test_guidance_without_the_conditioning_it_masks_is_a_value_error():
    z = torch.zeros(2, 1, 8, 8, 8)
    s, v = torch.zeros(2, 1, 8, 8, 8), [torch.zeros(2, 6)]
    m = _vdm(_net(), w_cfg=1.0, cfg_drop="vs").eval().model
    with pytest.raises(ValueError, match="v_conditionings"):
        m.get_pred_noise(z, m.gamma(torch.tensor(0.5)), s_conditioning=s)
    with pytest.raises(ValueError, match="v_conditionings"):
        m.sample(2, 2, "cpu", s_conditioning=s)
    ms = _vdm(_net(), w_cfg=1.0, cfg_drop="s").eval().model
    with pytest.raises(ValueError, match="s_conditioning"):
        ms.get_pred_noise(z, ms.gamma(torch.tensor(0.5)), v_conditionings=v)


def test_cabi_entries_refuse_bad_arguments_without_a_launch(hip_lib):
    """Host library only (as test_cabi_argument_errors_do_not_need_a_gpu): VDM_ERR_ARG = -1 and a message, nothing is launched.  The
    pointers are fake, suitably aligned addresses that a launch would fault on."""
    L, A = hip_lib, 4096
    nan = float("nan")
    for args, word in (((0.5, 1, None, 0, 4, None, None), b"NULL"), ((0.5, 1, None, 0, 0, A, None), b"rows"),
                       ((0.5, 1, None, 0, -3, A, None), b"rows"), ((-0.01, 1, None, 0, 4, A, None), b"[0, 1]"),
                       ((1.01, 1, None, 0, 4, A, None), b"[0, 1]"), ((nan, 1, None, 0, 4, A, None), b"[0, 1]"),
                       ((0.5, 1, None, 0, 4, A + 2, None), b"aligned"), ((0.5, 1, A + 1, 0, 4, A, None), b"aligned")):
        assert L.vdm_cond_keep(*args) == -1 and word in L.vdm_last_error(), (args, L.vdm_last_error())
    for args, word in (((None, A, 3, 4, A, None), b"NULL"), ((A, None, 3, 4, A, None), b"NULL"), ((A, A, 3, 4, None, None), b"NULL"),
                       ((A, A, 0, 4, A, None), b"rows"), ((A, A, 3, 0, A, None), b"dim"), ((A + 2, A, 3, 4, A, None), b"aligned"),
                       ((A, A + 1, 3, 4, A, None), b"aligned"), ((A, A, 3, 4, A + 3, None), b"aligned")):
        assert L.vdm_mask_rows(*args) == -1 and word in L.vdm_last_error(), (args, L.vdm_last_error())

    def head(x=A, cond=A, k=2, eps=None, step=None, alpha=A, sigma=A, n=3, per=64, dtype=0, z=A, packed=A, keep=A):
        return L.vdm_diffuse_pack_fields_keep(x, cond, k, eps, 1, 2, step, alpha, sigma, n, per, dtype, z, packed, keep, None)
    for kw, word in (({"x": None}, b"NULL"), ({"cond": None}, b"NULL"), ({"alpha": None}, b"NULL"), ({"sigma": None}, b"NULL"),
                     ({"packed": None}, b"NULL"), ({"k": 0}, b"1 to 3"), ({"k": 4}, b"1 to 3"), ({"n": 0}, b"sizes"), ({"per": 0}, b"sizes"),
                     ({"per": 66}, b"multiple of 4"), ({"dtype": 2}, b"dtype"), ({"x": A + 4}, b"aligned"), ({"cond": A + 8}, b"aligned"),
                     ({"packed": A + 4}, b"aligned"), ({"keep": A + 2}, b"aligned"), ({"alpha": A + 1}, b"aligned"),
                     ({"keep": None, "k": 5}, b"1 to 3")):
        assert head(**kw) == -1 and word in L.vdm_last_error(), (kw, L.vdm_last_error())


# ------------------------------------------------------------------------------------------ torch backend
def _batch(B=4, K=1):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 1, 8, 8, 8, generator=g)
    s = torch.randn(B, K, 8, 8, 8, generator=g) if K else None
    v = [torch.rand(B, 6, generator=g)]
    return x, s, v


def _masked(t, keep):
    return t * keep.view((-1,) + (1,) * (t.dim() - 1))


@pytest.mark.parametrize("K,drop", [(0, "v"), (1, "vs")])
def test_torch_backend_training_step_equals_the_masked_inputs(K, drop):
    """p_uncond = 0.5: get_loss equals get_loss of a p_uncond = 0 model on the inputs masked by last_cond_keep, from the same generator
    states (the keep is the first draw of the rank's noise generator: the reference model's generator is advanced by one rand(B))."""
    from vdm4cdm_amd import vdm_model as vm
    B = 4
    x, s, v = _batch(B, K)
    kw = lambda s_, v_: {"v_conditionings": v_, **({"s_conditioning": s_} if K else {})}
    torch.manual_seed(SEED)
    vm.reset_train_generators()
    a = _vdm(_net(K), p_uncond=0.5, cfg_drop=drop).train()
    la, _ = a.model.get_loss(x, **kw(s, v))
    keep = a.model.last_cond_keep
    assert keep.shape == (B,) and keep.dtype == torch.float32 and set(keep.tolist()) == {0.0, 1.0}, keep      # both fates in this batch
    torch.manual_seed(SEED)
    vm.reset_train_generators()
    b = _vdm(_net(K)).train()
    torch.rand(B, generator=b.model._rank_noise_gen("cpu", 0))
    lb, _ = b.model.get_loss(x, **kw(_masked(s, keep) if ("s" in drop and K) else s, [_masked(v[0], keep)] if "v" in drop else v))
    assert b.model.last_cond_keep is None and torch.equal(la, lb), (la, lb)
    la.backward()
    lb.backward()
    assert torch.equal(a.model.score_model.flat.grad, b.model.score_model.flat.grad)
    # the mask matters (else the comparison above would show nothing)
    torch.manual_seed(SEED)
    vm.reset_train_generators()
    c = _vdm(_net(K)).train()
    torch.rand(B, generator=c.model._rank_noise_gen("cpu", 0))
    lc, _ = c.model.get_loss(x, **kw(s, v))
    assert not torch.equal(la, lc)


def test_eval_mode_and_p_zero_never_drop():
    x, s, v = _batch()
    m = _vdm(_net(), p_uncond=0.5, cfg_drop="vs").eval()
    with torch.no_grad():
        m.validation_step({"x": x, "conditioning": s, "conditioning_values": v})
    assert m.model.last_cond_keep is None
    m0 = _vdm(_net()).train()
    m0.training_step({"x": x, "conditioning": s, "conditioning_values": v})
    assert m0.model.last_cond_keep is None and m0.rng_state_dict().get("cond_keep_calls") is None
    d = _vdm(_net(), p_uncond=1.0, cfg_drop="vs").train()                  # p = 1 drops every row, p -> 0+ keeps (rand > p)
    d.training_step({"x": x, "conditioning": s, "conditioning_values": v})
    assert not d.model.last_cond_keep.any()


def test_guidance_on_the_field_is_the_blend_with_the_zero_cube():
    """w_cfg with cfg_drop="s": (1 + w) net(z, s, v) - w net(z, 0, v) - the v rows of the unguided half are not masked - within the
    tolerance of test_cfg_pred_noise_and_sampler_on_torch_backend (1e-4)."""
    w = 1.5
    x, s, v = _batch(2)
    net = _net()
    m = _vdm(net, w_cfg=w, cfg_drop="s").eval().model
    with torch.no_grad():
        g_t = m.gamma(torch.tensor(0.4))
        tn = torch.full((2,), 0.4)
        e = m.get_pred_noise(x, g_t, s_conditioning=s, v_conditionings=v)
        e_c, e_u = net(x, t=tn, s_conditioning=s, v_conditionings=v), net(x, t=tn, s_conditioning=torch.zeros_like(s), v_conditionings=v)
        e_v = net(x, t=tn, s_conditioning=torch.zeros_like(s), v_conditionings=[torch.zeros_like(v[0])])
        assert (e_c - e_u).abs().max().item() > 1e-3 and (e_u - e_v).abs().max().item() > 1e-3
        assert (e - ((1 + w) * e_c - w * e_u)).abs().max().item() < 1e-4
        mvs = _vdm(net, w_cfg=w, cfg_drop="vs").eval().model
        e2 = mvs.get_pred_noise(x, g_t, s_conditioning=s, v_conditionings=v)
        assert (e2 - ((1 + w) * e_c - w * e_v)).abs().max().item() < 1e-4


# ------------------------------------------------------------------------------------------ knobs
def _config(**kw):
    return {"type": "VDM", "ckpt_path": None, "in_field_name": "Mstar", "out_field_name": "Mcdm", "cropsize": 8, "chs": [8, 16], **kw}


def test_get_model_guidance_knobs(monkeypatch, tmp_path, capsys):
    from vdm4cdm_amd import utils
    for k in ("VDM4CDM_W_CFG", "VDM4CDM_CFG_DROP"):
        monkeypatch.delenv(k, raising=False)
    m = utils.get_model(_config(), backend="torch")
    assert m.model.w_cfg is None and m.model.cfg_drop == "v" and "WARNING" not in capsys.readouterr().out
    # a checkpoint that records its conditioning dropout: cfg_drop comes from it, no warning
    path = str(tmp_path / "a.ckpt")
    torch.save({"state_dict": m.state_dict(), "global_step": 1, "epoch": 0, "cfg_dropout": {"p_uncond": 0.1, "cfg_drop": "vs"}}, path)
    g = utils.get_model(_config(ckpt_path=path, w_cfg=1.0), backend="torch")
    assert g.model.w_cfg == 1.0 and g.model.cfg_drop == "vs" and "WARNING" not in capsys.readouterr().out
    monkeypatch.setenv("VDM4CDM_W_CFG", "0.5")                               # the environment wins over the config key
    monkeypatch.setenv("VDM4CDM_CFG_DROP", "s")
    g = utils.get_model(_config(ckpt_path=path, w_cfg=1.0), backend="torch")
    assert g.model.w_cfg == 0.5 and g.model.cfg_drop == "s"
    # guidance from weights that never saw the null token: one loud line, and the run goes on
    monkeypatch.delenv("VDM4CDM_CFG_DROP")
    capsys.readouterr()
    g = utils.get_model(_config(), backend="torch")
    out = capsys.readouterr().out
    assert g.model.w_cfg == 0.5 and g.model.cfg_drop == "v" and out.count("WARNING") == 1 and "p_uncond" in out
    torch.save({"state_dict": m.state_dict(), "global_step": 1, "epoch": 0, "cfg_dropout": {"p_uncond": 0.0, "cfg_drop": "v"}}, path)
    utils.get_model(_config(ckpt_path=path), backend="torch")
    assert capsys.readouterr().out.count("WARNING") == 1


def test_get_model_refuses_bad_knobs_before_building_a_model(monkeypatch):
    from vdm4cdm_amd import networks, utils

    def no_model(*a, **k):
        raise AssertionError("the model must not be built")
    monkeypatch.setattr(networks, "CUNet", no_model)
    for k in ("VDM4CDM_W_CFG", "VDM4CDM_CFG_DROP"):
        monkeypatch.delenv(k, raising=False)
    for cfg in (_config(w_cfg="much"), _config(w_cfg=float("nan")), _config(w_cfg=1.0, cfg_drop="sv")):
        with pytest.raises(ValueError, match="w_cfg|cfg_drop"):
            utils.get_model(cfg, backend="torch")
    monkeypatch.setenv("VDM4CDM_W_CFG", "1e400x")
    with pytest.raises(ValueError, match="VDM4CDM_W_CFG"):
        utils.get_model(_config(), backend="torch")
    monkeypatch.setenv("VDM4CDM_W_CFG", "1.0")
    monkeypatch.setenv("VDM4CDM_CFG_DROP", "both")
    with pytest.raises(ValueError, match="VDM4CDM_CFG_DROP"):
        utils.get_model(_config(), backend="torch")


def test_training_script_knobs(monkeypatch):
    from vdm4cdm_amd import entry
    for k in ("VDM4CDM_P_UNCOND", "VDM4CDM_CFG_DROP"):
        monkeypatch.delenv(k, raising=False)
    assert entry._cfg_dropout_kwargs() == {"p_uncond": 0.0, "cfg_drop": "v"}
    monkeypatch.setenv("VDM4CDM_P_UNCOND", "0.1")
    monkeypatch.setenv("VDM4CDM_CFG_DROP", "vs")
    assert entry._cfg_dropout_kwargs() == {"p_uncond": 0.1, "cfg_drop": "vs"}
    for name, bad in (("VDM4CDM_P_UNCOND", "1.5"), ("VDM4CDM_P_UNCOND", "ten"), ("VDM4CDM_P_UNCOND", "nan"), ("VDM4CDM_CFG_DROP", "sv")):
        monkeypatch.setenv("VDM4CDM_P_UNCOND", "0.1")
        monkeypatch.setenv("VDM4CDM_CFG_DROP", "vs")
        monkeypatch.setenv(name, bad)
        with pytest.raises(SystemExit, match="p_uncond|cfg_drop"):
            entry._cfg_dropout_kwargs()


def test_checkpoints_record_the_dropout_and_resume_refuses_another(tmp_path):
    """A checkpoint written by fit carries {"p_uncond", "cfg_drop"} next to the trainer state; fit(ckpt_path=) of a model with other
    values is a ValueError that names both, before any training work; the host call counter travels in rng_state_dict()."""
    from vdm4cdm_amd import data
    from vdm4cdm_amd.trainer import Trainer

    def run(p, drop, steps, ckpt=None, name="a"):
        torch.manual_seed(3)
        from vdm4cdm_amd import vdm_model as vm
        vm.reset_train_generators()
        dm = data.SyntheticAstroDataModule(cropsize=8, batch_size=2, dim=3, channel_names=["Mstar", "Mcdm"], conditioning=True, n_params=6)
        m = _vdm(_net(), p_uncond=p, cfg_drop=drop)
        tr = Trainer(max_steps=steps, val_check_interval=0, every_n_train_steps=2, default_root_dir=str(tmp_path), experiment_name=name,
                     device="cpu", enable_progress=False)
        tr.fit(m, dm, ckpt_path=ckpt)
        return m, tr
    m, tr = run(0.5, "vs", 2)
    path = str(tmp_path / "a" / "checkpoints" / "epoch=0-step=2.ckpt")
    ck = torch.load(path, map_location="cpu")
    assert ck["cfg_dropout"] == {"p_uncond": 0.5, "cfg_drop": "vs"} and "trainer_state" in ck
    with pytest.raises(ValueError, match=r"p_uncond=0\.5.*p_uncond=0\.25"):
        run(0.25, "vs", 4, ckpt=path)
    with pytest.raises(ValueError, match="cfg_drop='vs'.*cfg_drop='s'"):
        run(0.5, "s", 4, ckpt=path)
    run(0.5, "vs", 3, ckpt=path)                                           # the same values: the run continues
