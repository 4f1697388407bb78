"""CPU tests of the normalisation step (vdm_log_moments, data.merge_log_moments / field_normalization / calc_normalizations,
calc_normalization.py, VDM4CDM_NORMALIZATIONS): the C-ABI surface and its argument errors, the merge arithmetic against numpy, the
environment variable in AstroDataModule (constants, errors, checkpoint state), and the errors the tool raises before any GPU work."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from _normalization_cases import checker, small_root, values, write_stack

ERR_ARG = -1
PTR = C.c_void_p(4096)                       # a non-NULL address that is never dereferenced: every call below returns before a launch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEL = {"dataset_name": "CMD", "suite_name": "Astrid", "set_name": "LH", "z_name": "z_0.0"}
MGAS = (9.4321987654321, 0.61234567891234)   # made-up constants, every digit of a float64 in use
MCDM = (10.123456789012345, 0.5012345678901234)


def test_log_moments_entry_is_exported_and_rejects_bad_arguments(hip_lib):
    from vdm4cdm_amd import _lib, hip_ops
    assert "vdm_log_moments" in _lib.SIGNATURES and hasattr(hip_lib, "vdm_log_moments")
    f = hip_lib.vdm_log_moments
    inf, nan = math.inf, math.nan
    for args, word in [((None, 8, 1.0, 0.0, PTR, PTR, None), b"x is NULL"), ((PTR, 8, 1.0, 0.0, None, PTR, None), b"out is NULL"),
                       ((PTR, 8, 1.0, 0.0, PTR, None, None), b"workspace is NULL"), ((PTR, -1, 1.0, 0.0, PTR, PTR, None), b"n = -1"),
                       ((PTR, 8, inf, 0.0, PTR, PTR, None), b"alpha"), ((PTR, 8, nan, 0.0, PTR, PTR, None), b"alpha"),
                       ((PTR, 8, 1.0, -inf, PTR, PTR, None), b"pivot"), ((PTR, 8, 1.0, nan, PTR, PTR, None), b"pivot"),
                       ((None, 0, 1.0, 0.0, PTR, PTR, None), b"x is NULL")]:
        assert f(*args) == ERR_ARG, args
        assert word in hip_lib.vdm_last_error(), (args, hip_lib.vdm_last_error())
    # the ABI number and the two sizes agree in header, binding and library
    header = open(os.path.join(ROOT, "include", "vdm4cdm_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (VDM_ABI_VERSION|VDM_LOG_MOMENTS_OUT|VDM_LOG_MOMENTS_WS)\s+(\d+)", header)}
    assert defs["VDM_ABI_VERSION"] == _lib.ABI_VERSION == hip_lib.vdm_abi_version() and _lib.ABI_VERSION >= 17
    assert (defs["VDM_LOG_MOMENTS_OUT"], defs["VDM_LOG_MOMENTS_WS"]) == (hip_ops.LOG_MOMENTS_OUT, hip_ops.LOG_MOMENTS_WS)
    assert defs["VDM_LOG_MOMENTS_WS"] % defs["VDM_LOG_MOMENTS_OUT"] == 0


@pytest.mark.parametrize("kind,alpha", [("cdm", 1.0), ("star", 1.0)])
def test_merge_arithmetic_matches_numpy(kind, alpha):
    """merge_log_moments alone: the per-record S1 / S2 come from numpy in float64 (2^20 values split into 1, 3 and 64 records), so only
    the merge is under test - fsum of the records, mean = pivot + S1/N, std = sqrt(S2/N - (S1/N)^2) - to 1e-13 relative."""
    from vdm4cdm_amd import data
    x = values(kind, 2 ** 20)
    v = np.log10(x.astype(np.float64) + alpha)
    ref = checker(x, alpha)
    assert ref["mean"] == v.mean() and ref["std"] == v.std() and ref["n"] == 2 ** 20
    pivot = float(v[0])
    for parts in (1, 3, 64):
        recs = [{"n_valid": len(c), "S1": float((c - pivot).sum()), "S2": float(((c - pivot) ** 2).sum()), "min": float(xc.min()),
                 "max": float(xc.max()), "n_bad": 0} for c, xc in zip(np.array_split(v, parts), np.array_split(x, parts))]
        n, mean, std, lo, hi, n_bad = data.merge_log_moments(recs, pivot)
        print(f"{kind} / {parts} records: mean err {abs(mean - ref['mean']):.2e}, std err {abs(std - ref['std']):.2e}")
        assert (n, lo, hi, n_bad) == (2 ** 20, float(x.min()), float(x.max()), 0)
        assert abs(mean - ref["mean"]) <= 1e-13 * abs(ref["mean"]) and abs(std - ref["std"]) <= 1e-13 * ref["std"]
    # bad counts add; no valid element: NaN constants and the empty extremes
    n, mean, std, lo, hi, n_bad = data.merge_log_moments([{"n_valid": 0, "S1": 0.0, "S2": 0.0, "min": math.inf, "max": -math.inf,
                                                            "n_bad": 2}] * 2, 0.0)
    assert (n, lo, hi, n_bad) == (0, math.inf, -math.inf, 4) and math.isnan(mean) and math.isnan(std)
    assert data.merge_log_moments([{"n_valid": 2, "S1": 0.0, "S2": 0.0, "min": 1.0, "max": 1.0, "n_bad": 0}], 0.25)[1:3] == (0.25, 0.0)


def _module(data, root, names=("Mgas", "Mcdm"), **kw):
    return data.AstroDataModule(selection=SEL, channel_names=list(names), return_func=None, stage="fit", batch_size=2, do_crop=True,
                                cropsize=8, data_root=root, seed=3, **kw)


def _norm_file(path, **consts):
    flat = {}
    for field, (m, s) in consts.items():
        flat[f"{field}_m"], flat[f"{field}_s"] = m, s
    with open(path, "w") as fh:
        json.dump(flat, fh)
    return str(path)


def test_environment_variable_supplies_constants(tmp_path, monkeypatch, capsys):
    from vdm4cdm_amd import data
    root = small_root(tmp_path / "root")
    # without the variable: the KeyError of before, now saying what to do
    monkeypatch.delenv(data.NORMALIZATIONS_ENV, raising=False)
    with pytest.raises(KeyError, match="Mgas") as e:
        _module(data, root)
    assert "calc_normalization.py" in str(e.value) and data.NORMALIZATIONS_ENV in str(e.value)
    # a file that names only Mgas: Mgas from the file, Mcdm keeps the built-in constants
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, _norm_file(tmp_path / "gas.json", Mgas=MGAS))
    capsys.readouterr()
    dm = _module(data, root)
    said = capsys.readouterr().out
    assert said.count("[data]") == 1 and "Mgas" in said and "gas.json" in said
    assert dm.means == [MGAS[0], data.NORMALIZATIONS["Mcdm"][0]] and dm.stds == [MGAS[1], data.NORMALIZATIONS["Mcdm"][1]]
    assert dm.alphas == [1.0, 1.0] and dm._dev_fields is None, "the module was not built on the CPU"
    # a field with built-ins is overridden too (Mcdm re-derived for another suite): one line per field taken from the file
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, _norm_file(tmp_path / "both.json", Mgas=MGAS, Mcdm=MCDM, T=(4.0, 1.0)))
    dm = _module(data, root)
    assert capsys.readouterr().out.count("[data]") == 2
    assert dm.means == [MGAS[0], MCDM[0]] and dm.stds == [MGAS[1], MCDM[1]]
    # norm_func / unnorm_func use them and are inverse to each other in float64
    rho = torch.tensor(np.concatenate([[0.0, 1e-3, 1.0], values("cdm", 64).astype(np.float64)]), dtype=torch.float64)
    y = torch.linspace(-4.0, 4.0, 33, dtype=torch.float64)
    for i, (m, s) in enumerate((MGAS, MCDM)):
        assert torch.equal(dm.norm_func(rho, i), (torch.log10(rho + 1.0) - m) / s)
        back = dm.unnorm_func(dm.norm_func(rho, i), i)
        assert back.dtype == torch.float64 and ((back - rho).abs() <= 1e-12 * (rho + 1.0)).all()
        assert ((dm.norm_func(dm.unnorm_func(y, i), i) - y).abs() <= 1e-12).all()
    # still no constants anywhere: KeyError, naming the file's fields as well
    with pytest.raises(KeyError, match="HI") as e:
        _module(data, root, names=("HI", "Mcdm"))
    assert "calc_normalization.py" in str(e.value) and "both.json" in str(e.value)


@pytest.mark.parametrize("content,word", [
    (None, "cannot be read"), ("{not json", "cannot be read"), ("[1.0, 2.0]", "flat object"), ('{"Mgas": {"m": 1.0, "s": 2.0}}', "not a number"),
    ('{"Mgas_m": "9.4", "Mgas_s": 0.6}', "not a number"), ('{"Mgas_m": 9.4}', "without 'Mgas_s'"), ('{"Mgas_s": 0.6}', "without 'Mgas_m'"),
    ('{"Mgas_m": NaN, "Mgas_s": 0.6}', "not finite"), ('{"Mgas_m": 9.4, "Mgas_s": Infinity}', "not finite"),
    ('{"Mgas_m": 9.4, "Mgas_s": 0.0}', "positive"), ('{"Mgas_m": 9.4, "Mgas_s": -0.6}', "positive"),
    ('{"Mgas_m": 9.4, "Mgas_s": 0.6, "comment": 1}', "neither")])
def test_malformed_normalisation_file_is_a_value_error(tmp_path, monkeypatch, content, word):
    from vdm4cdm_amd import data
    root = small_root(tmp_path / "root")
    path = tmp_path / "bad.json"
    if content is not None:
        path.write_text(content)
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, str(path))
    with pytest.raises(ValueError, match=word):
        _module(data, root)
    with pytest.raises(ValueError, match=word):                  # also where every field has built-in constants: the file is the user's word
        _module(data, root, names=("Mcdm", "Mcdm"))


def test_unset_variable_changes_nothing(tmp_path, monkeypatch, capsys):
    from vdm4cdm_amd import data
    monkeypatch.delenv(data.NORMALIZATIONS_ENV, raising=False)
    root = data.write_synthetic_camels(str(tmp_path / "r"), "CMD", fullsize=16, n_sims=2)
    capsys.readouterr()
    dm = _module(data, root, names=("Mstar", "Mcdm"))
    assert "[data]" not in capsys.readouterr().out
    assert dm.means == [0.010429391444558287, 10.019186475678042] and dm.stds == [0.3219291117577123, 0.5520203178284999]
    sd = dm.state_dict()
    assert set(sd) == {"kind", "seed", "nsamples", "batch_size", "crop", "stage", "epoch_gen_state", "aug_generators"}
    assert (sd["kind"], sd["seed"], sd["nsamples"], sd["batch_size"], sd["crop"], sd["stage"]) == ("AstroDataModule", 3, 16, 2, 8, "fit")
    _module(data, root, names=("Mstar", "Mcdm")).load_state_dict(sd)


def test_state_dict_records_file_constants(tmp_path, monkeypatch):
    from vdm4cdm_amd import data
    root = small_root(tmp_path / "root")
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, _norm_file(tmp_path / "a.json", Mgas=MGAS))
    a = _module(data, root)
    sd = a.state_dict()
    assert sd["norm"] == [[1.0, MGAS[0], MGAS[1]], [1.0, *data.NORMALIZATIONS["Mcdm"]]]
    _module(data, root).load_state_dict(sd)                      # the same constants: accepted
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, _norm_file(tmp_path / "b.json", Mgas=(MGAS[0], MGAS[1] * (1 + 1e-15))))
    b = _module(data, root)
    with pytest.raises(ValueError, match="norm") as e:
        b.load_state_dict(sd)
    assert "does not match" in str(e.value)
    old = {k: v for k, v in sd.items() if k != "norm"}          # a state written before the key existed, or by a default run
    b.load_state_dict(old)
    # a default module refuses a saved run whose recorded constants are not its own, and accepts one whose constants are
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, _norm_file(tmp_path / "c.json", Mcdm=MCDM))
    c = _module(data, root, names=("Mcdm", "Mcdm"))
    same = _norm_file(tmp_path / "d.json", Mcdm=data.NORMALIZATIONS["Mcdm"])
    monkeypatch.delenv(data.NORMALIZATIONS_ENV)
    d = _module(data, root, names=("Mcdm", "Mcdm"))
    assert "norm" not in d.state_dict()
    with pytest.raises(ValueError, match="norm"):
        d.load_state_dict(c.state_dict())
    monkeypatch.setenv(data.NORMALIZATIONS_ENV, same)
    d.load_state_dict(_module(data, root, names=("Mcdm", "Mcdm")).state_dict())


def test_tool_refuses_before_any_gpu_work(tmp_path, monkeypatch):
    import calc_normalization as cli
    from vdm4cdm_amd import data, hip_ops

    def no_launch(*a, **k):
        raise AssertionError("vdm_log_moments was reached: the error must come first")

    monkeypatch.setattr(hip_ops, "log_moments", no_launch)
    root = small_root(tmp_path / "root")
    out = tmp_path / "n.json"
    write_stack(root, "T", np.ones((2, 16, 16, 8), np.float32))
    write_stack(root, "Vgas", np.ones((2, 16, 16, 16), np.float32))
    cases = [(dict(field="HI"), ["HI"], "does not exist"), (dict(field="T"), ["T"], "not a stack of cubes"),
             (dict(field="Vgas"), ["Vgas"], "alpha"), (dict(field="Mgas", suite="SIMBA"), ["Mgas", "--suite", "SIMBA"], "SIMBA"),
             (dict(field="Mgas", nside=128), ["Mgas", "--nside", "128"], "3D_grids_128")]
    monkeypatch.setenv(data.DATA_ROOT_ENV, root)
    for kw, argv, word in cases:
        with pytest.raises(ValueError, match=word):
            data.field_normalization(root, device="cpu", **kw)
        with pytest.raises(ValueError, match=word):
            cli.main(argv + ["--out", str(out)])
    with pytest.raises(ValueError, match="CAMELS directory"):
        data.field_normalization(None, "Mgas", device="cpu")
    with pytest.raises(ValueError, match="not finite"):
        data.field_normalization(root, "Mgas", alpha=math.inf, device="cpu")
    # one bad field refuses the whole command line, whatever its position; a malformed --out is refused as well
    with pytest.raises(ValueError, match="does not exist"):
        cli.main(["Mgas", "HI", "--out", str(out)])
    out.write_text('{"Mcdm_m": 1.0}')
    with pytest.raises(ValueError, match="without 'Mcdm_s'"):
        cli.main(["Mgas", "--out", str(out)])
    assert out.read_text() == '{"Mcdm_m": 1.0}' and sorted(os.listdir(tmp_path)) == ["n.json", "root"]
    monkeypatch.delenv(data.DATA_ROOT_ENV)
    with pytest.raises(SystemExit):
        cli.main(["Mgas"])
    # with everything in order the pass itself needs a GPU: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        data.field_normalization(root, "Mgas", device="cpu")
