"""GPU tests of the down-gridding step: the HIP kernel (vdm_downgrid_trilinear) against the float64 checker of
tests/_downgrid_checker.py at every ratio of the real sizes, the exact cases, determinism, the tool (data.make_down_grids and the
command line) end to end, and the data module that derives the resampled set in HBM against the one that reads the written files."""
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _downgrid_checker import check_downgrid, interpolate_bound, kernel_bound, lognormal_cubes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(x, T):
    from vdm4cdm_amd import hip_ops as ops
    out = ops.downgrid_trilinear(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), T)
    assert out.shape == (len(x), T, T, T) and out.dtype == torch.float32
    return out.cpu().numpy()


def _worst(out, ref, bound):
    """largest |out - ref| / bound over ALL voxels (a voxel with a zero bound must be exact)"""
    err = np.abs(out.astype(np.float64) - ref)
    assert np.isfinite(out).all() and out.shape == ref.shape
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)).max())


@pytest.mark.parametrize("T", [8, 10, 11, 12, 14, 16])
def test_kernel_matches_checker_at_every_ratio(T):
    """n = 3, S = 16: the ratios 2, 8/5, 16/11, 4/3, 8/7, 1 of 256 -> 128, 160, 176, 192, 224, 256; T = 10, 11, 14 take the scalar path,
    the others the 16-byte one; first and last planes are the clamped ones; n > 1 checks the stack stride.  Every voxel is compared."""
    x = lognormal_cubes(3, 16, seed=T)
    ref, lo, hi, amax = check_downgrid(x, T)
    ratio = _worst(_run(x, T), ref, kernel_bound(amax))
    print(f"kernel 16->{T}: worst |err| / (16 2^-24 max|corner|) = {ratio:.3f}")
    assert ratio <= 1.0


def test_exact_cases_and_axis_order():
    rng = np.random.default_rng(1)
    x = lognormal_cubes(3, 16, seed=2)
    x[0, 0, 0, :4] = [-0.0, 0.0, -1.5, 3e38]
    assert np.array_equal(_run(x, 16).view(np.uint32), x.view(np.uint32)), "T == S is not a bit-exact copy"
    odd = lognormal_cubes(2, 13, seed=3)                     # the scalar path at T == S
    assert np.array_equal(_run(odd, 13).view(np.uint32), odd.view(np.uint32))
    v = rng.integers(-(2 ** 20) + 1, 2 ** 20, (3, 16, 16, 16)).astype(np.float32)
    mean = v.astype(np.float64).reshape(3, 8, 2, 8, 2, 8, 2).mean(axis=(2, 4, 6))
    assert np.array_equal(_run(v, 8).astype(np.float64), mean), "16 -> 8 of integers is not the 2x2x2 mean"
    ramp = np.arange(16, dtype=np.float32) * 3.0 + 1.0
    for axis in (1, 2, 3):                                   # linear in z, then y, then x only: swapped axes cannot pass
        shape = [1, 1, 1, 1]
        shape[axis] = 16
        lin = np.ascontiguousarray(np.broadcast_to(ramp.reshape(shape), (2, 16, 16, 16)))
        for T in (11, 12):
            ref, lo, hi, amax = check_downgrid(lin, T)
            out = _run(lin, T)
            assert _worst(out, ref, kernel_bound(amax)) <= 1.0, (axis, T)
            assert (np.diff(out, axis=axis) > 0).all(), (axis, T)


def test_vector_path_at_the_real_size_256_to_224():
    x = lognormal_cubes(1, 256, seed=4)
    out = _run(x, 224)
    ref, lo, hi, amax = check_downgrid(x, 224)
    ratio = _worst(out, ref, kernel_bound(amax))
    y = F.interpolate(torch.from_numpy(x)[:, None], size=224, mode="trilinear", align_corners=False)[:, 0].numpy()
    vs_torch = _worst(out, y.astype(np.float64), interpolate_bound(256, lo, hi, amax))
    torch_ratio = _worst(y, ref, interpolate_bound(256, lo, hi, amax))
    print(f"kernel 256->224: worst |err| / bound = {ratio:.3f}; F.interpolate vs checker {torch_ratio:.3f}; kernel vs F.interpolate "
          f"{vs_torch:.3f}")
    assert ratio <= 1.0 and torch_ratio <= 1.0
    assert vs_torch <= 1.0                                   # within the CPU-test bound of F.interpolate itself


def test_equal_bits_on_every_call_and_stream():
    from vdm4cdm_amd import hip_ops as ops
    x = torch.from_numpy(lognormal_cubes(3, 16, seed=5)).to(DEV)
    big = torch.from_numpy(lognormal_cubes(1, 64, seed=6)).to(DEV)
    for src, T in ((x, 11), (x, 12), (big, 56)):
        a = ops.downgrid_trilinear(src, T)
        b = ops.downgrid_trilinear(src, T, out=torch.full_like(a, float("nan")))
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = ops.downgrid_trilinear(src, T)
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c), T
    assert ops.downgrid_trilinear(x[:0], 8).shape == (0, 8, 8, 8)
    with pytest.raises(Exception, match="exceeds S"):
        ops.downgrid_trilinear(x, 17)


def _stamp(path):
    st = os.stat(path)
    return st.st_ino, st.st_mtime_ns


def _batch_fields(b):
    return [b["x"], b["conditioning"], b["conditioning_values"][0]]


def test_tool_end_to_end_and_derived_module_equals_files(tmp_path, monkeypatch, capsys):
    import make_down_grids as cli
    from vdm4cdm_amd import data, hip_ops as ops
    root = data.write_synthetic_camels(str(tmp_path / "root"), "CMD", fullsize=16, n_sims=4)
    only256 = shutil.copytree(root, str(tmp_path / "only256"))
    rep = data.make_down_grids(root, 128, sets=["LH"], device=DEV)
    targets = [data.field_path(root, "CMD_128", "Astrid", "LH", "z_0.0", c) for c in ("Mcdm", "Mstar")]
    assert [r["path"] for r in rep] == targets and all(r["status"] == "written" for r in rep)
    for c, p in zip(("Mcdm", "Mstar"), targets):
        assert p.endswith(os.path.join("3D_grids_128", f"Grids_{c}_Astrid_LH_128_z=0.0.npy"))
        got = np.load(p)
        src = torch.from_numpy(np.load(data.field_path(root, "CMD", "Astrid", "LH", "z_0.0", c))).to(DEV)
        assert got.shape == (4, 8, 8, 8) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), ops.downgrid_trilinear(src, 8).cpu().numpy().view(np.uint32))
    assert sorted(os.listdir(os.path.dirname(targets[0]))) == sorted(os.path.basename(p) for p in targets), "a temporary file is left"
    # a second call keeps the files; --overwrite (the command line) rewrites them
    before = [_stamp(p) for p in targets]
    assert all(r["status"] == "kept" for r in data.make_down_grids(root, 128, sets=["LH"], device=DEV))
    assert [_stamp(p) for p in targets] == before
    monkeypatch.setenv(data.DATA_ROOT_ENV, root)
    cli.main(["128", "--sets", "LH"])
    assert [_stamp(p) for p in targets] == before
    content = [np.load(p) for p in targets]
    cli.main(["128", "--sets", "LH", "--overwrite"])
    assert all(a != b for a, b in zip([_stamp(p) for p in targets], before))
    assert all(np.array_equal(np.load(p), c) for p, c in zip(targets, content))
    assert sorted(os.listdir(os.path.dirname(targets[0]))) == sorted(os.path.basename(p) for p in targets)
    monkeypatch.delenv(data.DATA_ROOT_ENV)

    # module A reads the written CMD_128 files, module B derives them in HBM from the 256 stack alone
    def module(r):
        return data.get_dataset(dataset_name="CMD_128", channel_names=["Mstar", "Mcdm"], stage="fit", batch_size=2, cropsize=4,
                                data_root=r, seed=11, device=DEV,
                                return_func=lambda fields, params: {"conditioning": fields[0], "x": fields[1], "conditioning_values": [params]})

    monkeypatch.delenv(data.DOWNGRID_ENV, raising=False)
    a = module(root)
    assert not os.path.exists(os.path.join(only256, "3D_grids_128"))
    monkeypatch.setenv(data.DOWNGRID_ENV, "1")
    capsys.readouterr()
    b = module(only256)
    assert "derived" in capsys.readouterr().out and b._derived_edge == [8, 8] and a._derived_edge == [None, None]
    assert (a.fullsize, a.ncrops, a.nsamples) == (b.fullsize, b.ncrops, b.nsamples) == (8, 8, 32)
    ta, tb, va, vb = iter(a.train_dataloader()), iter(b.train_dataloader()), iter(a.val_dataloader()), iter(b.val_dataloader())
    for la, lb in ((ta, tb), (ta, tb), (va, vb)):
        for u, v in zip(_batch_fields(next(la)), _batch_fields(next(lb))):
            assert u.shape == v.shape and torch.equal(u, v)
    assert all(torch.equal(u, v) for u, v in zip(a._dev_fields, b._dev_fields)) and b._dev_fields[0].shape == (4, 8, 8, 8)
