"""CPU tests of the down-gridding step (vdm_downgrid_trilinear, data.make_down_grids, VDM4CDM_DOWNGRID): the C-ABI surface and its
argument errors, the target-size rule, the opt-in selection in AstroDataModule - and a statement about the reference's own function,
F.interpolate(mode="trilinear", align_corners=False), against the float64 checker of tests/_downgrid_checker.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _downgrid_checker import check_downgrid, interpolate_bound, lognormal_cubes, taps

ERR_ARG = -1
PTR = C.c_void_p(4096)                       # a non-NULL address that is never dereferenced: every call below returns before a launch


def test_downgrid_entry_is_exported_and_rejects_bad_arguments(hip_lib):
    from vdm4cdm_amd import _lib
    assert "vdm_downgrid_trilinear" in _lib.SIGNATURES and hasattr(hip_lib, "vdm_downgrid_trilinear")
    f = hip_lib.vdm_downgrid_trilinear
    for args, word in [((None, PTR, 1, 16, 8, None), b"src"), ((PTR, None, 1, 16, 8, None), b"dst"), ((PTR, PTR, -1, 16, 8, None), b"n ="),
                       ((PTR, PTR, 1, 8, 16, None), b"exceeds S"), ((PTR, PTR, 1, 0, 0, None), b"S = 0"),
                       ((PTR, PTR, 1, 1025, 8, None), b"S = 1025"), ((PTR, PTR, 1, 16, 0, None), b"T = 0"),
                       ((PTR, PTR, 1, 16, -4, None), b"T = -4")]:
        assert f(*args) == ERR_ARG, args
        assert word in hip_lib.vdm_last_error(), (args, hip_lib.vdm_last_error())
    assert f(PTR, PTR, 0, 16, 8, None) == 0                  # n == 0: a successful no-op, nothing is launched
    assert f(PTR, PTR, 0, 1024, 1024, None) == 0


def test_checker_is_the_block_mean_at_ratio_two_and_the_identity_at_ratio_one():
    x = np.random.default_rng(0).integers(-1000, 1000, (2, 16, 16, 16)).astype(np.float32)
    ref, lo, hi, amax = check_downgrid(x, 8)
    assert np.array_equal(ref, x.astype(np.float64).reshape(2, 8, 2, 8, 2, 8, 2).mean(axis=(2, 4, 6)))
    assert np.array_equal(hi, x.reshape(2, 8, 2, 8, 2, 8, 2).max(axis=(2, 4, 6))) and (amax >= np.abs(ref)).all() and (lo <= ref).all()
    assert np.array_equal(check_downgrid(x, 16)[0], x)
    i0, i1, lam = taps(256, 224)                             # first / last plane: the coordinate 1/14 and 255 - 1/14, nothing clamped away
    assert (i0[0], i1[0], i0[-1], i1[-1]) == (0, 1, 254, 255) and lam[0] == 32 / 448 and lam[-1] == 416 / 448
    assert taps(16, 16)[2].max() == 0 and taps(3, 1)[0][0] == 1


@pytest.mark.parametrize("S,T,n", [(16, 8, 3), (16, 10, 3), (16, 11, 3), (16, 12, 3), (16, 14, 3), (16, 16, 3), (64, 56, 1)])
def test_reference_interpolate_stays_within_the_fp32_coordinate_bound(S, T, n):
    """The reference's own resampler, on CPU fp32, against the exact-ratio checker: within 6 S 2^-24 (max8 - min8) + 24 2^-24 max|corner|
    (2 S 2^-24 of lambda uncertainty per axis from the fp32 coordinate, times the corner range, plus the blend's rounding)."""
    x = lognormal_cubes(n, S, seed=S * 1000 + T)
    y = F.interpolate(torch.from_numpy(x)[:, None], size=T, mode="trilinear", align_corners=False)[:, 0].numpy()
    ref, lo, hi, amax = check_downgrid(x, T)
    ratio = (np.abs(y - ref) / interpolate_bound(S, lo, hi, amax)).max()
    print(f"F.interpolate {S}->{T}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_target_edge_rule_and_value_errors(tmp_path):
    from vdm4cdm_amd import data
    assert [data.down_grid_edge(n, 256) for n in (128, 160, 176, 192, 224, 256, 1)] == [128, 160, 176, 192, 224, 256, 1]
    assert [data.down_grid_edge(n, 16) for n in (128, 160, 176, 192, 224)] == [8, 10, 11, 12, 14] and data.down_grid_edge(128, 32) == 16
    for nside, s_file, word in [(0, 256, "1..256"), (257, 256, "1..256"), (-128, 256, "1..256"), (128.0, 256, "1..256"),
                                (100, 16, "non-integer"), (8, 16, "non-integer")]:
        with pytest.raises(ValueError, match=word):
            data.down_grid_edge(nside, s_file)
    # make_down_grids checks everything before it touches a GPU (there is none here): a bad nside, a non-integer edge, a missing source
    root = data.write_synthetic_camels(str(tmp_path / "r"), "CMD", fullsize=16, n_sims=2)
    with pytest.raises(ValueError, match="1..256"):
        data.make_down_grids(root, 300, sets=["LH"])
    with pytest.raises(ValueError, match="non-integer"):
        data.make_down_grids(root, 100, sets=["LH"])
    with pytest.raises(ValueError, match="Grids_Mcdm_Astrid_CV_256") as e:
        data.make_down_grids(root, 128)                      # the default sets: the CV stack is not there
    assert "does not exist" in str(e.value)
    with pytest.raises(ValueError, match="SIMBA"):
        data.make_down_grids(root, 128, sets=["LH"], suite="SIMBA")
    with pytest.raises(ValueError, match="CAMELS directory"):
        data.make_down_grids(None, 128)
    assert not os.path.exists(os.path.join(root, "3D_grids_128")), "a refused call wrote something"
    # an existing target is left alone (no GPU work either)
    kept = [data.field_path(root, "CMD_128", "Astrid", "LH", "z_0.0", c) for c in ("Mcdm", "Mstar")]
    os.makedirs(os.path.dirname(kept[0]))
    for p in kept:
        np.save(p, np.zeros((2, 8, 8, 8), np.float32))
    rep = data.make_down_grids(root, 128, sets=["LH"], verbose=False)
    assert [r["status"] for r in rep] == ["kept", "kept"] and [r["path"] for r in rep] == kept and rep[0]["shape"] == (2, 8, 8, 8)
    assert sorted(os.listdir(os.path.dirname(kept[0]))) == sorted(os.path.basename(p) for p in kept)


def _module(data, root, **kw):
    return data.get_dataset(dataset_name="CMD_128", channel_names=["Mstar", "Mcdm"], stage="fit", batch_size=2, cropsize=4,
                            data_root=root, seed=5, **kw)


def test_downgrid_opt_in_selection(tmp_path, monkeypatch, capsys):
    """VDM4CDM_DOWNGRID: unset -> FileNotFoundError as before; set and the 256 stack present -> the module of the resampled set (fullsize
    = T, same anchors, crops and split as the file-backed one); set and the resampled file present -> the file wins; no source -> error."""
    from vdm4cdm_amd import data
    root = data.write_synthetic_camels(str(tmp_path / "only256"), "CMD", fullsize=16, n_sims=4)
    monkeypatch.delenv(data.DOWNGRID_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match="3D_grids_128"):
        _module(data, root)
    monkeypatch.setenv(data.DOWNGRID_ENV, "0")               # only "1" opts in
    with pytest.raises(FileNotFoundError, match="3D_grids_128"):
        _module(data, root)
    monkeypatch.setenv(data.DOWNGRID_ENV, "1")
    capsys.readouterr()
    dm = _module(data, root)
    said = capsys.readouterr().out
    assert said.count("derived") == 2 and "Grids_Mcdm_Astrid_LH_256_z=0.0.npy" in said
    assert dm.fullsize == 8 and dm._derived_edge == [8, 8] and dm.fields[0].shape == (4, 16, 16, 16)
    # the same module as one over files of the resampled size
    files = data.write_synthetic_camels(str(tmp_path / "files"), "CMD_128", fullsize=8, n_sims=4)
    fm = _module(data, files)
    assert (dm.fullsize, dm.crop, dm.ncrops, dm.nsamples) == (fm.fullsize, fm.crop, fm.ncrops, fm.nsamples) == (8, 4, 8, 32)
    assert np.array_equal(dm.anchors, fm.anchors) and dm.train_idx == fm.train_idx and dm.valid_idx == fm.valid_idx
    sa, sb = dm.state_dict(), fm.state_dict()
    assert {k: v for k, v in sa.items() if not isinstance(v, (torch.Tensor, dict))} == \
        {k: v for k, v in sb.items() if not isinstance(v, (torch.Tensor, dict))}
    fm.load_state_dict(sa)                                   # a checkpoint of the derived run resumes on the file-backed set
    # the resampled file is there: it wins, knob or not (here it has another size than the rule would give, to tell them apart)
    data.write_synthetic_camels(root, "CMD_128", fullsize=12, n_sims=4)
    capsys.readouterr()
    dm = _module(data, root)
    assert dm.fullsize == 12 and dm._derived_edge == [None, None] and "derived" not in capsys.readouterr().out
    # no 256 stack to derive from
    empty = data.write_synthetic_camels(str(tmp_path / "other"), "CMD_160", fullsize=10, n_sims=4)
    with pytest.raises(FileNotFoundError, match="3D_grids_new"):
        _module(data, empty)
    # the 256 data set itself is never "derived"
    with pytest.raises(FileNotFoundError):
        data.get_dataset(dataset_name="CMD", channel_names=["Mstar", "Mcdm"], cropsize=4, data_root=empty)
