"""Learned-linear training on the HIP backend, the parts that need no GPU: the two train3D entry points (command line, settings) and the
argument checks of the C-ABI entries behind the network's input gradients (K1t vdm_conv_in_dgrad, K7b vdm_schedule_grad_sums, K6i
vdm_cond_input_grad)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ["train3D_c_c_from_field_name.py", "train3D_c_c_from_field_name_160.py"]


@pytest.mark.parametrize("script", SCRIPTS)
def test_train3d_scripts_exist_and_reject_wrong_arity(script):
    path = os.path.join(ROOT, script)
    assert os.path.exists(path)
    for args in ([], ["Mstar"], ["Mstar", "Mcdm", "128"]):
        r = subprocess.run([sys.executable, path] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "usage" in (r.stderr + r.stdout), (args, r.stderr[-400:])


def test_train3d_variant_table_holds_the_reference_values():
    from vdm4cdm_amd import entry
    assert entry.TRAIN3D_VARIANTS == {"128": (128, "LH_c_uc_{i}_to_{o}", 16), "160": (160, "LH_c_uc_{i}_to_{o}_160", 20)}
    c = entry.TRAIN3D_COMMON
    assert (c["dataset_name"], c["suite_name"], c["set_name"]) == ("CMD", "Astrid", "LH")
    assert c["batch_size"] == 2 and c["chs"] == [48, 96, 192, 384] and c["conditioning_values"] == 6 and c["norm_groups"] == 8
    assert c["dropout_prob"] == 0.1 and c["conv_padding_mode"] == "zeros"
    assert c["noise_schedule"] == "learned_linear" and (c["gamma_min"], c["gamma_max"]) == (-13.3, 13.3)
    assert c["val_check_interval"] == 1000 and c["every_n_train_steps"] == 10_000 and c["gradient_clip_val"] == 0.5
    assert c["learning_rate"] == 3.0e-4
    assert entry.TRAIN3D_VARIANTS["128"][1].format(i="Mstar", o="Mcdm") == "LH_c_uc_Mstar_to_Mcdm"


def test_conv_in_dgrad_argument_errors(hip_lib):
    L = hip_lib
    ok = dict(dh=4096, n=1, d=8, h=8, w=8, c=32, dtype=1, pad=0, weight=4096, cin=2, dz=4096, ds=8192)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vdm_conv_in_dgrad(a["dh"], a["n"], a["d"], a["h"], a["w"], a["c"], a["dtype"], a["pad"], a["weight"], a["cin"], a["dz"],
                                   a["ds"], None)

    assert call(dh=None) == -1 and b"NULL" in L.vdm_last_error()
    assert call(dz=None) == -1 and b"NULL" in L.vdm_last_error()
    assert call(c=24) == -1 and b"out of range" in L.vdm_last_error()
    assert call(c=128) == -1 and b"out of range" in L.vdm_last_error()
    assert call(cin=3) == -1 and b"out of range" in L.vdm_last_error()
    assert call(cin=1) == -1 and b"ds needs" in L.vdm_last_error()
    assert call(d=0) == -1 and b"bad grid" in L.vdm_last_error()
    assert call(dtype=7) == -1 and b"dtype" in L.vdm_last_error()
    assert call(pad=5) == -1 and b"pad_mode" in L.vdm_last_error()
    assert call(dh=4104) == -1 and b"aligned" in L.vdm_last_error()
    assert call(dz=4098) == -1 and b"aligned" in L.vdm_last_error()


def test_schedule_grad_sums_argument_errors(hip_lib):
    L = hip_lib

    def call(dz=4096, x=8192, eps=None, n=2, per=64, sums=4096, ws=4096):
        return L.vdm_schedule_grad_sums(dz, x, eps, 1, 1, None, n, per, sums, ws, None)

    assert call(dz=None) == -1 and b"NULL" in L.vdm_last_error()
    assert call(sums=None) == -1 and b"NULL" in L.vdm_last_error()
    assert call(per=66) == -1 and b"multiple of 4" in L.vdm_last_error()
    assert call(n=0) == -1 and b"bad sizes" in L.vdm_last_error()
    assert call(x=8200) == -1 and b"aligned" in L.vdm_last_error()
    assert call(eps=8196) == -1 and b"aligned" in L.vdm_last_error()


def test_reduction_entries_refuse_more_samples_than_workspace_rows(hip_lib):
    """The two-stage reductions write one partial row per block into a workspace of 2048 rows whose size the C ABI never sees; with more
    than 2048 samples even one block per sample overruns it, so the three entries refuse (before any launch)."""
    L = hip_lib
    for n in (2049, 100000):
        assert L.vdm_schedule_grad_sums(4096, 8192, None, 1, 1, None, n, 64, 4096, 4096, None) == -1
        assert b"schedule_grad_sums: at most 2048 samples" in L.vdm_last_error()
        assert L.vdm_loss_terms(4096, 4096, 4096, 4096, 1.0, 4096, n, 64, 4096, 4096, 4096, None) == -1
        assert b"loss_terms: at most 2048 samples" in L.vdm_last_error()
        assert L.vdm_loss_terms_rng(4096, None, 1, 1, 4096, None, 2, 2, None, 1.0, 4096, n, 64, 4096, 4096, 4096, None) == -1
        assert b"loss_terms_rng: at most 2048 samples" in L.vdm_last_error()


def test_cond_input_grad_argument_errors(hip_lib):
    from vdm4cdm_amd._lib import CondMlp
    L = hip_lib
    mlps = (CondMlp * 2)()
    for k, (in_dim, dim, sin) in enumerate(((64, 128, 1), (6, 64, 0))):
        m = mlps[k]
        m.input, m.in_dim, m.dim, m.sinusoid = 4096, in_dim, dim, sin
        m.w1, m.b1, m.w2, m.b2, m.wproj = 4096, 4096, 4096, 4096, 4096
    outs = (C.c_void_p * 2)(8192, None)
    assert L.vdm_cond_input_grad(mlps, 2, 2, 1312, None, 4096, outs, None) == -1 and b"NULL" in L.vdm_last_error()
    assert L.vdm_cond_input_grad(mlps, 2, 2, 1312, 4096, 4096, None, None) == -1 and b"NULL" in L.vdm_last_error()
    assert L.vdm_cond_input_grad(mlps, 9, 2, 1312, 4096, 4096, outs, None) == -1               # more than 4 conditionings
    assert L.vdm_cond_input_grad(mlps, 2, 70000, 1312, 4096, 4096, outs, None) == -1 and b"65535" in L.vdm_last_error()
    bad = (C.c_void_p * 2)(8194, None)
    assert L.vdm_cond_input_grad(mlps, 2, 2, 1312, 4096, 4096, bad, None) == -1 and b"aligned" in L.vdm_last_error()
    mlps[1].in_dim = 300
    assert L.vdm_cond_input_grad(mlps, 2, 2, 1312, 4096, 4096, outs, None) == -1 and b"out of range" in L.vdm_last_error()
    mlps[1].in_dim = 6
    mlps[0].w1 = None
    assert L.vdm_cond_input_grad(mlps, 2, 2, 1312, 4096, 4096, outs, None) == -1 and b"NULL" in L.vdm_last_error()
