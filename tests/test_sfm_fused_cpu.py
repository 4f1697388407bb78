"""Host side of the fused flow-matching step (ABI v21): the two C entries in the header and the binding, their argument refusals (every
one comes before a launch, so no device is needed - the pointers are never dereferenced), the wrappers' own refusals, the optimizer
hook's signature, and the torch backend, which did not move."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vdm_sfm_head", "vdm_sfm_loss")


def _header():
    with open(os.path.join(ROOT, "include", "vdm4cdm_hip.h")) as f:
        return f.read()


def _declared_params(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vdm4cdm_hip.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_and_binding_declare_both_entries_at_abi_21():
    from vdm4cdm_amd import _lib
    header = _header()
    assert int(re.search(r"#define VDM_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 21
    for name in ENTRIES:
        params = _declared_params(header, name)
        assert len(params) == len(_lib.SIGNATURES[name][1]), (name, params)
        assert params[-1] == "void* stream"
    head = _declared_params(header, "vdm_sfm_head")
    assert [p.split()[-1].lstrip("*") for p in head] == ["x0", "x1", "eps", "seed", "stream_id", "seed_step", "t", "sigma", "cond", "n", "per",
                                                         "dtype", "x_t", "packed", "stream"]
    loss = _declared_params(header, "vdm_sfm_loss")
    assert [p.split()[-1].lstrip("*") for p in loss] == ["v_hat", "x0", "x1", "coef", "n", "per", "sums", "d_v", "workspace", "stream"]
    assert _lib.lib().vdm_abi_version() == 21


A16, A4 = 0x10000, 0x20004          # a 16-byte aligned and a merely 4-byte aligned address (never dereferenced: every call is refused)


def test_head_entry_refuses_bad_arguments_on_the_host():
    from vdm4cdm_amd import _lib
    L = _lib.lib()
    good = dict(x0=A16, x1=A16, eps=A16, seed=1, sid=1, step=None, t=A4, sigma=0.1, cond=1, n=2, per=260, dtype=0, x=A16, packed=A16)
    bad = [("x0", None, "NULL"), ("x1", None, "NULL"), ("t", None, "NULL"), ("packed", None, "NULL"), ("per", 258, "multiple of 4"),
           ("per", 0, "bad sizes"), ("n", 0, "bad sizes"), ("dtype", 2, "bad dtype"), ("sigma", -1e-3, "sigma"), ("sigma", float("nan"), "sigma"),
           ("cond", 2, "cond"), ("x0", A4, "16-byte aligned"), ("x1", A4, "16-byte aligned"), ("eps", A4, "16-byte aligned"),
           ("x", A4, "16-byte aligned"), ("packed", A4, "16-byte aligned"), ("t", A16 + 2, "4-byte aligned"), ("step", A16 + 1, "4-byte aligned")]
    for key, value, msg in bad:
        a = {**good, key: value}
        rc = L.vdm_sfm_head(a["x0"], a["x1"], a["eps"], a["seed"], a["sid"], a["step"], a["t"], a["sigma"], a["cond"], a["n"], a["per"],
                            a["dtype"], a["x"], a["packed"], None)
        err = L.vdm_last_error().decode()
        assert rc == -1 and err.startswith("sfm_head:") and msg in err, (key, value, rc, err)


def test_loss_entry_refuses_bad_arguments_on_the_host():
    from vdm4cdm_amd import _lib
    L = _lib.lib()
    good = dict(vh=A16, x0=A16, x1=A16, coef=A4, n=2, per=260, sums=A4, dv=A16, ws=A4)
    bad = [(k, None, "NULL") for k in ("vh", "x0", "x1", "coef", "sums", "dv", "ws")] + \
          [("per", 258, "multiple of 4"), ("per", -4, "bad sizes"), ("n", 0, "bad sizes"), ("n", 2049, "at most 2048 samples"),
           ("vh", A4, "16-byte aligned"), ("x0", A4, "16-byte aligned"), ("x1", A4, "16-byte aligned"), ("dv", A4, "16-byte aligned"),
           ("coef", A16 + 2, "4-byte aligned")]
    for key, value, msg in bad:
        a = {**good, key: value}
        rc = L.vdm_sfm_loss(a["vh"], a["x0"], a["x1"], a["coef"], a["n"], a["per"], a["sums"], a["dv"], a["ws"], None)
        err = L.vdm_last_error().decode()
        assert rc == -1 and err.startswith("sfm_loss:") and msg in err, (key, value, rc, err)


def test_wrappers_refuse_a_voxel_count_that_is_no_multiple_of_4_before_touching_a_device():
    from vdm4cdm_amd import hip_ops as ops
    a, t = torch.zeros(2, 1, 3, 3, 2), torch.zeros(2)                       # 18 voxels per sample, CPU tensors
    with pytest.raises(ValueError, match="18 voxels per sample is not a multiple of 4"):
        ops.sfm_head(a, a, t, 0.0, torch.float32)
    with pytest.raises(ValueError, match="18 elements per sample is not a multiple of 4"):
        ops.sfm_loss(a, a, a, t, torch.zeros(2), torch.empty_like(a))
    assert list(inspect.signature(ops.sfm_head).parameters)[:10] == ["x0", "x1", "t", "sigma", "dtype", "cond", "eps", "seed", "stream_id", "want_x"]
    assert list(inspect.signature(ops.sfm_loss).parameters) == ["v_hat", "x0", "x1", "coef", "sums", "d_v", "workspace"]


def _torch_sfm(sigma):
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.sfm_model import LightSFM
    net = CUNet(shape=(1, 8, 8, 8), chs=[8, 16], s_conditioning_channels=1, v_conditioning_dims=[6], t_conditioning=True, norm_groups=8,
                mid_attn=False, dropout_prob=0.0, conv_padding_mode="zeros", n_attention_heads=4, backend="torch", precision="fp32")
    net.reset_parameters(generator=torch.Generator().manual_seed(21), zero_init_std=0.05)
    return LightSFM(velocity_model=net, learning_rate=3e-4, sigma=sigma).train()


def test_configure_optimizers_accepts_capturable_and_installs_the_repack_hook():
    from vdm4cdm_amd.sfm_model import LightSFM
    from vdm4cdm_amd.trainer import _accepts
    assert _accepts(LightSFM.configure_optimizers, "capturable")
    assert inspect.signature(LightSFM.configure_optimizers).parameters["capturable"].default is False
    sfm = _torch_sfm(0.0)
    vm, calls = sfm.model.velocity_model, []
    vm.mark_weights_dirty = lambda: calls.append("dirty")
    vm.repack_weights = lambda: calls.append("repack")
    opt = sfm.configure_optimizers(capturable=True)                          # (CPU parameters: neither fused nor capturable)
    assert opt.param_groups[0]["capturable"] is False
    for p in sfm.parameters():
        p.grad = torch.zeros_like(p)
    opt.step()
    assert calls == ["dirty", "repack"]
    assert sfm.model.graph_capturable() == (True, "")
    ok, why = LightSFM(velocity_model=vm, antithetic_time_sampling=False).model.graph_capturable()
    assert ok is False and "antithetic_time_sampling=False" in why


def test_batch_shapes_cover_every_tensor_of_a_batch():
    from vdm4cdm_amd.trainer import batch_shapes
    a = {"x0": torch.zeros(2, 1, 4, 4, 4), "x1": torch.zeros(2, 1, 4, 4, 4), "conditioning_values": [torch.zeros(2, 6)], "conditioning": None}
    assert batch_shapes(a) == {"x0": (2, 1, 4, 4, 4), "x1": (2, 1, 4, 4, 4), "conditioning_values": ((2, 6),), "conditioning": None}
    ragged = {**a, "x1": torch.zeros(1, 1, 4, 4, 4)}
    assert batch_shapes(ragged) != batch_shapes(a) and batch_shapes({**a, "conditioning_values": [torch.zeros(1, 6)]}) != batch_shapes(a)


@pytest.mark.parametrize("sigma", [0.0, 0.1])
def test_torch_backend_loss_is_the_parent_expression(sigma):
    """The torch backend's get_loss against a restatement of what it computed before the fused HIP path existed: same generators in the
    same order, the same bits in the loss and in every gradient."""
    import vdm4cdm_amd.vdm_model as vm
    sfm = _torch_sfm(sigma)
    g = torch.Generator().manual_seed(3)
    x0, x1, v = torch.randn(2, 1, 8, 8, 8, generator=g), torch.randn(2, 1, 8, 8, 8, generator=g), [torch.rand(2, 6, generator=g)]

    def reseed():
        torch.manual_seed(11)
        vm.reset_train_generators()
        for p in sfm.parameters():
            p.grad = None

    reseed()
    loss, metrics = sfm.model.get_loss(x0=x0, x1=x1, v_conditionings=v)
    loss.backward()
    got = [p.grad.clone() for p in sfm.parameters()]
    reseed()
    t = vm.stratified_times(2, x1.device, True)
    xt = (1.0 - t).view(2, 1, 1, 1, 1) * x0 + t.view(2, 1, 1, 1, 1) * x1
    if sigma > 0.0:
        xt = xt + sigma * torch.randn_like(x1)
    ref = ((sfm.model.velocity(xt, t, x0, v) - (x1 - x0)) ** 2).mean()
    ref.backward()
    assert torch.equal(loss.detach(), ref.detach()) and torch.equal(metrics["loss"], ref.detach())
    assert all(torch.equal(a, p.grad) for a, p in zip(got, sfm.parameters())) and got[0].abs().max().item() > 0
