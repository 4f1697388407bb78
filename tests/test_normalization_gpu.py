"""GPU tests of the normalisation step: the HIP kernel (vdm_log_moments) against the notebook's own arithmetic in numpy
(tests/_normalization_cases.py), the exact cases, determinism, slab independence of data.field_normalization, the tool
(calc_normalization.py) end to end, and a data module that trains on the constants the tool wrote."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from _normalization_cases import N_BIG, assert_moments_close, checker, small_root, values, write_stack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.array(a, np.float32)).to(DEV)     # (a copy: the shared inputs are read-only)


def _stats(t, alpha, pivot):
    """(record, (n, mean, std, min, max, n_bad)) of one kernel call on the device tensor t."""
    from vdm4cdm_amd import data, hip_ops as ops
    rec = ops.log_moments(t, alpha, pivot)
    return rec, data.merge_log_moments([rec], pivot)


@pytest.mark.parametrize("n", [1, 63, 64, 257, 4099, N_BIG])
@pytest.mark.parametrize("kind", ["cdm", "star"])
def test_kernel_matches_checker(kind, n):
    """Mean and std of one kernel call, merged by merge_log_moments, against np.log10(x.astype(np.float64) + alpha).mean() / .std() to
    1e-11 relative (a mean below 1 in magnitude: 1e-11 absolute); min, max and the two counts exactly.  n: a single lane, under and at
    one wave, one past a workgroup, a ragged vector tail, many grid-stride rounds with a tail; each with the pointer at the tensor's
    start (16-byte loads) and at element offset 1 (4-byte aligned only: the scalar loads), alpha 1 and 2, pivot = log10(x[0] + alpha).

    Where the 1e-11 comes from (derived, not tuned): everything is float64 - a few ulp of log10 per element plus the sequential
    accumulation of at most about 10^3 terms per thread stay below 1e-12 on mean and std.  Anything float32 in the chain lands at
    5e-8 to 2e-7 (measured on the CPU with these very inputs at n = 2^20: a float32 log10 gives 5.6e-8 on the mean and 2.0e-7 on the
    std, a float32 accumulation 5e-8).  1e-11 sits between the two with more than three decades on each side."""
    base = values(kind, N_BIG + 1)
    t = _dev(base[:n + 1])
    for off in (0, 1):
        x = base[off:off + n]
        assert t[off:off + n].data_ptr() % 16 == (0 if off == 0 else 4)
        for alpha in (1.0, 2.0):
            ref = checker(x, alpha)
            pivot = float(np.log10(np.float64(x[0]) + alpha))
            rec, (cnt, mean, std, lo, hi, n_bad) = _stats(t[off:off + n], alpha, pivot)
            assert (cnt, lo, hi, n_bad) == (n, ref["min"], ref["max"], 0) and rec["n_valid"] == n
            assert_moments_close(mean, std, ref, f"{kind} n={n} offset={off} alpha={alpha:g}")


def test_exact_cases():
    from vdm4cdm_amd import _lib, hip_ops as ops
    # all zeros, alpha = 1, pivot = 0: log10(1) = 0 exactly, so every sum is +0.0 bit for bit
    for n in (1, 4099, 2 ** 16 + 1):
        rec = ops.log_moments(torch.zeros(n, device=DEV), 1.0, 0.0)
        assert rec == {"n_valid": n, "S1": 0.0, "S2": 0.0, "min": 0.0, "max": 0.0, "n_bad": 0}
        assert [math.copysign(1.0, rec[k]) for k in ("S1", "S2", "min", "max")] == [1.0] * 4, "a negative zero"
    # NaN, +inf and two values with x + alpha <= 0 at four positions, the first and the last element among them
    x = values("cdm", 4099, seed=1).copy()
    where, bad = [0, 1234, 2049, 4098], [np.nan, np.inf, -3.0, -1.0]
    x[where] = bad
    keep = np.ones(len(x), bool)
    keep[where] = False
    ref, ref_kept = checker(x, 1.0), checker(x[keep], 1.0)
    assert ref["n_bad"] == 4 and ref["n"] == 4095 and (ref["mean"], ref["std"]) == (ref_kept["mean"], ref_kept["std"])
    for off in (0, 1):                                             # both load paths
        t = _dev(np.concatenate([np.zeros(off, np.float32), x]))[off:]
        rec, (cnt, mean, std, lo, hi, n_bad) = _stats(t, 1.0, 10.0)  # (x[0] is NaN: the pivot is a round number near the mean)
        assert (cnt, n_bad, lo, hi) == (4095, 4, float(x[keep].min()), float(x[keep].max())) and lo > 0 and math.isfinite(hi)
        assert_moments_close(mean, std, ref_kept, f"four bad elements, offset {off}")
    # -inf and a value that only alpha makes invalid
    rec = ops.log_moments(torch.tensor([-math.inf, -1.5, 0.0, 5.0], device=DEV), 1.5, 0.0)
    assert (rec["n_valid"], rec["n_bad"], rec["min"], rec["max"]) == (2, 2, 0.0, 5.0)
    # n == 0 with real device buffers: a successful call that writes the empty record
    buf = torch.full((ops.LOG_MOMENTS_OUT + ops.LOG_MOMENTS_WS,), math.nan, dtype=torch.float64, device=DEV)
    some = torch.ones(4, device=DEV)
    status = _lib.lib().vdm_log_moments(some.data_ptr(), 0, 1.0, 0.0, buf.data_ptr(), buf[ops.LOG_MOMENTS_OUT:].data_ptr(), None)
    torch.cuda.synchronize()
    assert status == 0 and buf[:ops.LOG_MOMENTS_OUT].tolist() == [0.0, 0.0, 0.0, math.inf, -math.inf, 0.0]
    assert ops.log_moments(some[:0], 1.0, 0.0) == {"n_valid": 0, "S1": 0.0, "S2": 0.0, "min": math.inf, "max": -math.inf, "n_bad": 0}


def test_equal_bits_on_every_call_and_alignment():
    """Two calls on the same 2^20 + 3 input give identical bytes in out (whatever the workspace held before); so does the same input
    behind a pointer that is only 4-byte aligned: the element-to-thread map does not depend on the load width."""
    from vdm4cdm_amd import _lib, hip_ops as ops
    base = values("cdm", N_BIG + 1)
    t = _dev(base[:N_BIG])
    shifted = _dev(np.concatenate([base[:1], base[:N_BIG]]))[1:]
    assert shifted.data_ptr() % 16 == 4 and torch.equal(shifted, t)
    outs = []
    for src, fill in ((t, 0.0), (t, math.nan), (shifted, 1e300)):
        buf = torch.full((ops.LOG_MOMENTS_OUT + ops.LOG_MOMENTS_WS,), fill, dtype=torch.float64, device=DEV)
        assert _lib.lib().vdm_log_moments(src.data_ptr(), N_BIG, 1.0, 10.0, buf.data_ptr(), buf[ops.LOG_MOMENTS_OUT:].data_ptr(),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        outs.append(buf[:ops.LOG_MOMENTS_OUT].cpu().numpy().tobytes())
    assert outs[0] == outs[1], "two calls on the same input differ"
    assert outs[0] == outs[2], "the result depends on the pointer's alignment"
    assert np.frombuffer(outs[0], np.float64)[0] == N_BIG


def test_field_normalization_is_independent_of_the_slabs(tmp_path):
    from vdm4cdm_amd import data
    cubes = values("cdm", 6 * 16 ** 3, seed=2).reshape(6, 16, 16, 16)
    root = str(tmp_path)
    path = write_stack(root, "Mgas", cubes)
    ref = checker(cubes, 1.0)
    got = [data.field_normalization(root, "Mgas", slab_sims=s, device=DEV) for s in (1, 4, None)]
    for s, r in zip((1, 4, None), got):
        assert r["n"] == 6 * 16 ** 3 and (r["min"], r["max"], r["alpha"], r["path"]) == (ref["min"], ref["max"], 1.0, path)
        assert set(r["seconds"]) == {"read", "h2d", "kernel"} and all(v >= 0 for v in r["seconds"].values())
        assert r["pivot"] == math.log10(float(cubes[0, 0, 0, 0]) + 1.0)
        assert_moments_close(r["mean"], r["std"], ref, f"slab_sims={s}")
    for r in got[1:]:                                              # and with each other, to the same bound
        assert abs(r["mean"] - got[0]["mean"]) <= 1e-11 * abs(ref["mean"]) and abs(r["std"] - got[0]["std"]) <= 1e-11 * ref["std"]
    # an explicit alpha; errors raised after the pass
    assert_moments_close(*[data.field_normalization(root, "Mgas", alpha=2.0, device=DEV)[k] for k in ("mean", "std")],
                         checker(cubes, 2.0), "alpha=2")
    write_stack(root, "HI", np.zeros((2, 16, 16, 16), np.float32))
    with pytest.raises(ValueError, match="std == 0"):
        data.field_normalization(root, "HI", device=DEV)


def test_tool_end_to_end_and_module_trains_on_its_constants(tmp_path, monkeypatch, capsys):
    import calc_normalization as cli
    from vdm4cdm_amd import data
    root = small_root(tmp_path / "root", n_sims=6)
    stacks = {c: np.load(data.field_path(root, "CMD", "Astrid", "LH", "z_0.0", c)) for c in ("Mgas", "Mcdm")}
    out = str(tmp_path / "f.json")
    monkeypatch.setenv(data.DATA_ROOT_ENV, root)
    monkeypatch.delenv(data.NORMALIZATIONS_ENV, raising=False)
    capsys.readouterr()
    cli.main(["Mgas", "--out", out])
    said = capsys.readouterr().out
    assert said.count("[calc_normalization]") == 1 and "Mgas" in said and "built-in" not in said
    first = json.load(open(out))
    assert sorted(first) == ["Mgas_m", "Mgas_s"]
    assert_moments_close(first["Mgas_m"], first["Mgas_s"], checker(stacks["Mgas"], 1.0), "tool Mgas")
    # a second run for another field keeps the entries of the first; a field with built-in constants reports its distance from them
    cli.main(["Mcdm", "--out", out])
    said = capsys.readouterr().out
    assert said.count("[calc_normalization]") == 1 and "built-in" in said
    both = json.load(open(out))
    assert sorted(both) == ["Mcdm_m", "Mcdm_s", "Mgas_m", "Mgas_s"] and {k: both[k] for k in first} == first
    assert_moments_close(both["Mcdm_m"], both["Mcdm_s"], checker(stacks["Mcdm"], 1.0), "tool Mcdm")
    assert data.load_normalizations(out) == {"Mgas": (both["Mgas_m"], both["Mgas_s"]), "Mcdm": (both["Mcdm_m"], both["Mcdm_s"])}
    # a failing field (a stack with a negative value: log10 undefined) leaves the old file as it was, and no temporary file
    bad = stacks["Mgas"].copy()
    bad[3, 2, 1, 0] = -7.5
    write_stack(root, "T", bad)
    before = open(out).read()
    with pytest.raises(ValueError, match="1 of 24576 elements") as e:
        cli.main(["T", "--out", out])
    assert "-7.5" in str(e.value) and "alpha = 1.0" in str(e.value)
    assert open(out).read() == before and sorted(os.listdir(tmp_path)) == ["f.json", "root"]
    # named fields are replaced (--alpha 2 gives other numbers), the others kept
    cli.main(["Mgas", "--alpha", "2", "--out", out])
    again = json.load(open(out))
    assert again["Mgas_m"] != both["Mgas_m"] and (again["Mcdm_m"], again["Mcdm_s"]) == (both["Mcdm_m"], both["Mcdm_s"])
    cli.main(["Mgas", "--out", out])
    assert json.load(open(out)) == both and sorted(os.listdir(tmp_path)) == ["f.json", "root"]

    # the module: with the file, Mgas -> Mcdm trains; the normalised Mgas channel of the whole test set has mean 0 and std 1.
    # 1e-4: the batch kernel computes log10 in float32, about 1e-7 relative on values near 10, divided by a std near 0.5 - a few 1e-6 per
    # element; constants that were not applied would leave a mean of order 10.
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, out)
    dm = data.AstroDataModule(selection={"dataset_name": "CMD", "suite_name": "Astrid", "set_name": "LH", "z_name": "z_0.0"},
                              channel_names=["Mgas", "Mcdm"], stage="test", batch_size=4, do_crop=False, device=DEV,
                              return_func=lambda fields, params: {"conditioning": fields[0], "x": fields[1], "conditioning_values": [params]})
    assert dm.means == [both["Mgas_m"], both["Mcdm_m"]] and dm.stds == [both["Mgas_s"], both["Mcdm_s"]]
    batches = list(dm.test_dataloader())
    gas = torch.cat([b["conditioning"] for b in batches]).double()
    cdm = torch.cat([b["x"] for b in batches]).double()
    assert gas.shape == cdm.shape == (6, 1, 16, 16, 16)
    for name, v in (("Mgas", gas), ("Mcdm", cdm)):
        m, s = v.mean().item(), v.std(unbiased=False).item()
        print(f"normalised {name}: mean {m:.3e}, std - 1 {s - 1:.3e}")
        assert abs(m) <= 1e-4 and abs(s - 1) <= 1e-4
