"""Exponential moving average of the weights, host side and torch backend (no GPU): the two C entries in the header, the binding and the
library with their refusals; constructor errors; the recurrence on a tiny CPU training run against tests/_ema_ref.py, bit for bit;
checkpoints, resume and its four refusals; validation under the averaged weights; the VDM4CDM_EMA_DECAY / VDM4CDM_WEIGHTS knobs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _ema_ref as R
import _resume_worker as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, DECAY = 12, 6, 0.5


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_weight_crosses_the_warmup_boundary():
    """(1 + k) / (10 + k) reaches 0.5 at k = 8: before it the warm-up value rules, from there on the decay."""
    ws = [float(R.weight(DECAY, True, k)) for k in range(12)]
    assert ws[0] == float(np.float32(1) - np.float32(1) / np.float32(10)) and ws[7] > 0.5 and ws[8:] == [0.5] * 4
    assert all(float(R.weight(DECAY, False, k)) == 0.5 for k in (0, 5, 1000))
    assert [R.roundings(DECAY, True, k) for k in (0, 8, 1000)] == [4 * ws[0] + 1, 3.0, 3.0] and R.roundings(0.0, False, 0) == 3.0
    from vdm4cdm_amd.ema import ema_weight
    for decay in R.DECAYS + [0.9999]:
        for warm in (True, False):
            for k in (0, 1, 7, 8, 9, 1000, 10 ** 6):
                assert ema_weight(decay, warm, k) == float(R.weight(decay, warm, k))


@pytest.mark.parametrize("n", R.SIZES)
def test_float32_reference_within_the_derived_bounds_of_float64(n):
    """The reference the kernel is pinned to meets, on the kernel test's own inputs, the bounds that test asserts (tests/_ema_ref.py)."""
    e, p = R.inputs(n)
    for decay in R.DECAYS:
        for warm in (True, False):
            for k in R.COUNTERS:
                got, want = R.ema_step(e, p, decay, warm, k or 0), R.ema_step64(e, p, decay, warm, k or 0)
                err = np.abs(got.astype(np.float64) - want)
                assert (err <= R.bound(e, p, got, decay, warm, k or 0)).all()
                assert (err <= R.bound_max(e, p, got, decay, warm, k or 0)).all()
                same = bits(e) == bits(p)                      # (-0 and +0 compare equal but -0 + w * (+0 - -0) is +0)
                assert np.array_equal(bits(got[same]), bits(e[same]))


# ------------------------------------------------------------------------------------------------ C-ABI surface
def test_entries_declared_bound_and_exported(hip_lib):
    from vdm4cdm_amd import _lib, hip_ops
    header = open(os.path.join(ROOT, "include", "vdm4cdm_hip.h")).read()
    assert re.search(r"int vdm_ema_update\(float\* ema, const float\* p, int64_t n, float decay, int warmup, const int32_t\* num_updates, "
                     r"void\* stream\);", header)
    assert re.search(r"int vdm_swap\(float\* a, float\* b, int64_t n, void\* stream\);", header)
    assert _lib.SIGNATURES["vdm_ema_update"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int, C.c_void_p, C.c_void_p])
    assert _lib.SIGNATURES["vdm_swap"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
    assert hasattr(hip_lib, "vdm_ema_update") and hasattr(hip_lib, "vdm_swap")
    assert callable(hip_ops.ema_update) and callable(hip_ops.swap_)
    assert int(re.search(r"#define VDM_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == hip_lib.vdm_abi_version()


def test_entries_refuse_bad_arguments_without_a_gpu(hip_lib):
    """Every refusal returns VDM_ERR_ARG (-1) with a message and launches nothing; n == 0 is VDM_OK.  The pointers are never followed:
    made-up addresses stand in for device memory."""
    L, a, b = hip_lib, 0x10000, 0x20000
    err = lambda: L.vdm_last_error().decode()
    assert L.vdm_ema_update(None, b, 4, 0.5, 1, None, None) == -1 and "NULL" in err()
    assert L.vdm_ema_update(a, None, 4, 0.5, 1, None, None) == -1 and "NULL" in err()
    assert L.vdm_ema_update(a, b, -1, 0.5, 1, None, None) == -1 and "n = -1" in err()
    for bad in (1.0, -0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        assert L.vdm_ema_update(a, b, 4, bad, 1, None, None) == -1 and "decay" in err()
    assert L.vdm_ema_update(a, a, 4, 0.5, 1, None, None) == -1 and "same vector" in err()
    assert L.vdm_ema_update(a, b, 0, 0.5, 1, None, None) == 0
    assert L.vdm_ema_update(a, b, 0, 0.0, 0, None, None) == 0
    assert L.vdm_swap(None, b, 4, None) == -1 and "NULL" in err()
    assert L.vdm_swap(a, None, 4, None) == -1 and "NULL" in err()
    assert L.vdm_swap(a, b, -3, None) == -1 and "n = -3" in err()
    assert L.vdm_swap(a, a, 4, None) == -1 and "overlap" in err()
    assert L.vdm_swap(a, a + 8, 4, None) == -1 and "overlap" in err()          # [a, a + 16) and [a + 8, a + 24)
    assert L.vdm_swap(a + 8, a, 4, None) == -1 and "overlap" in err()
    assert L.vdm_swap(a, a, 0, None) == -1 and "overlap" in err()
    assert L.vdm_swap(a, a + 16, 0, None) == 0


# ------------------------------------------------------------------------------------------------ construction
@pytest.mark.parametrize("bad", [1.0, -0.1, float("nan"), "x"], ids=["one", "negative", "nan", "string"])
def test_bad_decay_is_a_value_error_at_construction(bad):
    from vdm4cdm_amd.networks import CUNet
    from vdm4cdm_amd.sfm_model import LightSFM
    from vdm4cdm_amd.vdm_model import LightVDM
    net = CUNet(shape=(1, 8, 8, 8), chs=[8, 16], s_conditioning_channels=1, v_conditioning_dims=[6], norm_groups=4, backend="torch")
    with pytest.raises(ValueError, match="ema_decay"):
        LightVDM(score_model=net, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        LightSFM(velocity_model=net, ema_decay=bad)


def test_off_means_no_ema_object_and_a_noop_context():
    for decay in (None, 0, 0.0):
        vdm = R.make_vdm(ema_decay=decay)
        opt = vdm.configure_optimizers()
        assert vdm.ema is None and vdm.ema_decay is None and len(opt._optimizer_step_post_hooks) == 1
        before = vdm.model.score_model.flat.detach().clone()
        with vdm.ema_weights():
            assert torch.equal(vdm.model.score_model.flat, before)
    sfm = R.make_sfm()
    sfm.configure_optimizers()
    assert sfm.ema is None
    with sfm.ema_weights():
        pass
    assert set(R.make_vdm(ema_decay=0.9).state_dict()) == set(R.make_vdm().state_dict())       # the module's own keys are unchanged


# ------------------------------------------------------------------------------------------------ the recurrence on the torch backend
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Computed once: 12 CPU steps with EMA (decay 0.5, warm-up), the twin without, and the first leg of a stopped run."""
    root = tmp_path_factory.mktemp("ema_cpu")
    on = R.run_fit(root, "on", lambda: R.make_vdm(ema_decay=DECAY), N, every=N)
    off = R.run_fit(root, "off", lambda: R.make_vdm(), N)
    R.run_fit(root, "b", lambda: R.make_vdm(ema_decay=DECAY), K, every=K)
    return {"root": root, "on": on, "off": off, "ckpt": W.ckpt_at(root, "on", N), "ckpt_k": W.ckpt_at(root, "b", K)}


def test_shadow_follows_the_reference_and_training_is_untouched(runs):
    on, off = runs["on"], runs["off"]
    assert len(on["params"]) == N + 1 and on["num_updates"] == N and off["shadows"] is None
    R.assert_shadows_follow_ref(on, DECAY, True)
    assert not np.array_equal(on["shadows"][0], on["params"][-1][0])                     # (an average, not a copy)
    for a, b in zip(on["params"], off["params"]):                                         # the raw parameters: the same run, step by step
        assert np.array_equal(bits(a[0]), bits(b[0]))
    assert [h["loss"] for h in on["history"] if "loss" in h] == [h["loss"] for h in off["history"] if "loss" in h]


def test_learned_schedule_scalars_are_averaged_too(tmp_path):
    run = R.run_fit(tmp_path, "ll", lambda: R.make_vdm(schedule="learned_linear", ema_decay=DECAY, ema_warmup=False), 4)
    assert len(run["shadows"]) == 3 and [s.size for s in run["shadows"][1:]] == [1, 1]
    R.assert_shadows_follow_ref(run, DECAY, False)
    sd = run["model"].ema.state_dict()["shadow"]
    assert set(sd) == set(run["model"].state_dict()) and sd["model.gamma_b"].shape == ()


def test_swapped_restores_every_bit_and_does_not_nest():
    vdm = R.make_vdm(ema_decay=DECAY)
    vdm.configure_optimizers()
    ema, flat = vdm.ema, vdm.model.score_model.flat
    with torch.no_grad():
        flat.add_(1.0)
    ema.update()
    raw, shadow = flat.detach().clone(), ema.shadows[0].clone()
    assert not torch.equal(raw, shadow)
    with vdm.ema_weights():
        assert torch.equal(flat, shadow) and torch.equal(ema.shadows[0], raw)
        with pytest.raises(RuntimeError, match="re-entrant"):
            with vdm.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="swapped"):
            ema.update()
    assert torch.equal(flat, raw) and torch.equal(ema.shadows[0], shadow) and ema.num_updates == 1
    with pytest.raises(ZeroDivisionError):                      # an error inside still puts the weights back
        with vdm.ema_weights():
            1 / 0
    assert torch.equal(flat, raw) and torch.equal(ema.shadows[0], shadow)


# ------------------------------------------------------------------------------------------------ checkpoints and resume
def test_checkpoint_holds_the_average_under_the_models_keys(runs):
    ck = torch.load(runs["ckpt"], map_location="cpu")
    assert ck["ema"] == {"decay": DECAY, "warmup": True, "num_updates": N} and ck["trainer_state"]["format"] == 1
    assert set(ck["ema_state_dict"]) == set(ck["state_dict"])
    fresh = R.make_vdm()
    fresh.load_state_dict(ck["ema_state_dict"])
    assert np.array_equal(bits(fresh.model.score_model.flat.detach().numpy()), bits(runs["on"]["shadows"][0]))
    plain = torch.load(W.ckpt_at(runs["root"], "b", K), map_location="cpu")
    assert plain["ema"]["num_updates"] == K
    off_root = runs["root"] / "noema"
    R.run_fit(off_root, "x", lambda: R.make_vdm(), 2, every=2)
    assert not {"ema", "ema_state_dict"} & set(torch.load(W.ckpt_at(off_root, "x", 2), map_location="cpu"))


def test_ema_state_roundtrip_through_the_networks_layout_rules(runs):
    """load_state_dict goes through CUNet._convert_entry: the PyTorch conv layout [cout, cin, k, k, k] is accepted, a wrong shape is not."""
    src = runs["on"]["model"].ema
    state = src.state_dict()
    dst = R.make_vdm(ema_decay=DECAY)
    dst.configure_optimizers()
    torch_layout = dict(state["shadow"])
    k = "model.score_model.conv_in.weight"
    taps, cout, cin = torch_layout[k].shape
    torch_layout[k] = torch_layout[k].permute(1, 2, 0).reshape(cout, cin, 3, 3, 3).contiguous()
    dst.ema.load_state_dict({**state, "shadow": torch_layout})
    assert torch.equal(dst.ema.shadows[0], src.shadows[0]) and dst.ema.num_updates == N
    with pytest.raises(RuntimeError, match="expected"):
        dst.ema.load_state_dict({**state, "shadow": {**state["shadow"], k: state["shadow"][k].reshape(-1)}})
    with pytest.raises(ValueError, match="decay"):
        dst.ema.load_state_dict({**state, "decay": 0.25})


def test_resumed_run_is_the_uninterrupted_one(runs):
    b = R.run_fit(runs["root"], "b", lambda: R.make_vdm(ema_decay=DECAY), N, ckpt_path=runs["ckpt_k"])
    a = runs["on"]
    assert b["num_updates"] == a["num_updates"] == N and len(b["params"]) == N - K + 1
    assert np.array_equal(bits(b["shadows"][0]), bits(a["shadows"][0]))
    assert np.array_equal(bits(b["params"][-1][0]), bits(a["params"][-1][0]))
    ck = torch.load(runs["ckpt_k"], map_location="cpu")
    fresh = R.make_vdm()
    fresh.load_state_dict(ck["ema_state_dict"])               # the shadow the second leg started from
    R.assert_shadows_follow_ref(b, DECAY, True, k0=K, start=[fresh.model.score_model.flat.detach().numpy()])


def test_resume_refuses_an_ema_mismatch(runs, tmp_path):
    from vdm4cdm_amd.trainer import Trainer
    root = tmp_path
    R.run_fit(root, "plain", lambda: R.make_vdm(), 2, every=2)
    plain = W.ckpt_at(root, "plain", 2)

    def refit(path, match, **kw):
        W.fresh_process()
        vdm = R.make_vdm(**kw)
        vdm.to = None                                          # refused before the model is moved or anything else happens to it
        tr = Trainer(max_steps=N, default_root_dir=str(root), experiment_name="x", device="cpu", enable_progress=False)
        with pytest.raises(ValueError, match=match):
            tr.fit(vdm, R.make_dm(), ckpt_path=path)

    refit(plain, "holds no EMA", ema_decay=DECAY)
    refit(runs["ckpt_k"], "holds an EMA", ema_decay=None)
    refit(runs["ckpt_k"], "ema_decay=0.5 ema_warmup=True.*ema_decay=0.75", ema_decay=0.75)
    refit(runs["ckpt_k"], "ema_warmup=True.*ema_warmup=False", ema_decay=DECAY, ema_warmup=False)


# ------------------------------------------------------------------------------------------------ validation
def test_validation_uses_the_average_and_leaves_training_alone(tmp_path):
    """Two EMA runs and their twins without EMA, validation at steps 2 and 4 of 5: as far as the existing trainer goes (a validation pass
    draws from the training generators with or without EMA), the raw parameters of an EMA run are its twin's; the logged validation loss
    is the loss under ema_weights(), which differs from the loss of the raw weights."""
    on = R.run_fit(tmp_path, "on", lambda: R.make_vdm(ema_decay=DECAY), 5, val=2)
    off = R.run_fit(tmp_path, "off", lambda: R.make_vdm(), 5, val=2)
    for a, b in zip(on["params"], off["params"]):
        assert np.array_equal(bits(a[0]), bits(b[0]))
    R.assert_shadows_follow_ref(on, DECAY, True)
    v_on, v_off = W.losses(on["history"], key="val_loss"), W.losses(off["history"], key="val_loss")
    assert v_on.numel() == v_off.numel() == 2 and not torch.equal(v_on, v_off)

    # by hand: a third run of 4 steps without validation, then one validation pass from the same random streams three times - through
    # the trainer, under the context, and with the raw weights
    import contextlib
    from vdm4cdm_amd.trainer import rng_state, set_rng_state
    c = R.run_fit(tmp_path, "c", lambda: R.make_vdm(ema_decay=DECAY), 4)
    model, tr = c["model"], c["trainer"]
    streams, flat_before = rng_state(model, "cpu"), model.model.score_model.flat.detach().clone()

    def val_loss(inside):
        set_rng_state(model, "cpu", streams)
        with (model.ema_weights() if inside else contextlib.nullcontext()), torch.no_grad():
            model.eval()
            tot = [model.validation_step(b, i).float() * b["x"].shape[0] for i, b in enumerate(R.make_dm().val_dataloader()) if i < 2]
            model.train()
        return float(torch.stack(tot).sum() / 4)

    want_ema, want_raw = val_loss(True), val_loss(False)
    set_rng_state(model, "cpu", streams)
    rec = tr.validate(model, R.make_dm())
    assert rec["val_loss"] == want_ema and rec["val_samples"] == 4 and want_ema != want_raw
    assert torch.equal(model.model.score_model.flat, flat_before)


# ------------------------------------------------------------------------------------------------ entry points
def test_ema_decay_knob_is_checked_before_model_work(monkeypatch):
    from vdm4cdm_amd import entry, networks
    monkeypatch.setattr(networks, "CUNet", lambda *a, **k: pytest.fail("a model was built"))
    for bad in ("x", "1.0", "-0.1", "nan", "1e3"):
        monkeypatch.setenv("VDM4CDM_EMA_DECAY", bad)
        with pytest.raises(SystemExit, match="VDM4CDM_EMA_DECAY"):
            entry.train_vdm3d("128", ["Mstar", "Mcdm", "16"])
        with pytest.raises(SystemExit, match="VDM4CDM_EMA_DECAY"):
            entry.train_sfm3d("128", ["Mstar", "Mcdm", "16"])
    monkeypatch.setenv("VDM4CDM_EMA_DECAY", "0.9999")
    assert entry._ema_kwargs() == {"ema_decay": 0.9999}
    monkeypatch.setenv("VDM4CDM_EMA_DECAY", "0")
    assert entry._ema_kwargs() == {"ema_decay": None}
    monkeypatch.delenv("VDM4CDM_EMA_DECAY")
    assert entry._ema_kwargs() == {}


def _config(path):
    return {"type": "VDM", "cropsize": 16, "chs": [8, 16], "conditioning_values": 6, "ckpt_path": str(path), "precision": "fp32"}


def test_weights_knob(runs, tmp_path, monkeypatch, capsys):
    from vdm4cdm_amd import entry, networks, utils
    monkeypatch.delenv("VDM4CDM_WEIGHTS", raising=False)
    ck = torch.load(runs["ckpt"], map_location="cpu")
    raw_flat, ema_flat = runs["on"]["params"][-1][0], runs["on"]["shadows"][0]
    with_ema, without = _config(runs["ckpt"]), _config(tmp_path / "plain.ckpt")
    torch.save({k: ck[k] for k in ("state_dict", "global_step", "epoch")}, without["ckpt_path"])
    flat = lambda m: m.model.score_model.flat.detach().numpy()
    capsys.readouterr()
    # default: the average when the checkpoint has it, announced in one line; else the raw weights, silently
    assert np.array_equal(bits(flat(utils.get_model(with_ema, backend="torch"))), bits(ema_flat))
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "EMA" in out and "VDM4CDM_WEIGHTS=raw" in out
    assert np.array_equal(bits(flat(utils.get_model(without, backend="torch"))), bits(raw_flat))
    assert capsys.readouterr().out == ""
    # explicit, through the config key and through the environment (which wins)
    assert np.array_equal(bits(flat(utils.get_model({**with_ema, "weights": "raw"}, backend="torch"))), bits(raw_flat))
    assert np.array_equal(bits(flat(utils.get_model({**with_ema, "weights": "ema"}, backend="torch"))), bits(ema_flat))
    assert capsys.readouterr().out == ""
    monkeypatch.setenv("VDM4CDM_WEIGHTS", "ema")
    assert np.array_equal(bits(flat(utils.get_model({**with_ema, "weights": "raw"}, backend="torch"))), bits(ema_flat))
    with pytest.raises(ValueError, match="holds no ema_state_dict"):
        utils.get_model(without, backend="torch")
    with pytest.raises(ValueError, match="no checkpoint"):
        utils.get_model(_config(tmp_path / "nothing.ckpt"), backend="torch")
    # bad values: before any model work, in get_model and in the generate scripts
    monkeypatch.setattr(networks, "CUNet", lambda *a, **k: pytest.fail("a model was built"))
    monkeypatch.setenv("VDM4CDM_WEIGHTS", "average")
    with pytest.raises(ValueError, match="weights='average'"):
        utils.get_model(with_ema, backend="torch")
    for gen, runtype in ((entry.generate_3d, "CV_12_12"), (entry.generate_3d_1p, "1P_24")):
        with pytest.raises(SystemExit, match="VDM4CDM_WEIGHTS"):
            gen(["VDM_Mstar_Mcdm_c_c_128", str(tmp_path / "gen"), runtype])
    monkeypatch.delenv("VDM4CDM_WEIGHTS")
    with pytest.raises(ValueError, match="weights='both'"):
        utils.get_model({**with_ema, "weights": "both"}, backend="torch")
