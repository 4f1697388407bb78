"""VDM4CDM_EXPERIMENT, the one variable of the A/B and ablation switches: the strict Python parser (vdm4cdm_amd/_experiment.py), the
refusal of the retired variables, the module constants filled from it, the library's table and lenient parser (csrc/experiment.h), and
that every switch the host-side plan queries can see still changes the plans it is meant to change."""
import glob
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vdm4cdm_amd", "csrc")


def child(args, experiment=None, **env_extra):
    """A fresh interpreter in the repository root; no switch of the parent's environment reaches it."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("VDM4CDM_")}
    if experiment is not None:
        env["VDM4CDM_EXPERIMENT"] = experiment
    env.update(env_extra)
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)


# ---- 1. the parser ------------------------------------------------------------------------------
def test_parser_defaults_and_values():
    from vdm4cdm_amd import _experiment as ex
    defaults = {k: d for k, (d, _, _) in ex.TABLE.items()}
    assert len(defaults) == 19 and defaults["wgrad_wgs"] == 512 and defaults["grouped_reduce"] == 0 and defaults["ablate"] == set()
    for text in (None, "", " , ,,  ,"):
        assert ex.parse(text) == defaults, text
    got = ex.parse("split=0, ksplit=0,wgrad_wgs=256,ablate=wgrad+conv1,grouped_reduce")
    named = {"split": 0, "ksplit": 0, "wgrad_wgs": 256, "ablate": {"wgrad", "conv1"}, "grouped_reduce": 1}
    assert got == dict(defaults, **named)
    assert ex.parse("ablate=")["ablate"] == set()                    # tools/ablate_step.sh's "full step" line
    assert ex.parse("defer_wgrad_levels=0")["defer_wgrad_levels"] == 0 and ex.parse("wgrad_wgs=1")["wgrad_wgs"] == 1
    gn = ex.parse("fused_gn=0")
    assert gn["fused_gn"] == 0 and gn["fused_gnb"] == 0
    assert ex.parse("fused_gn=0,fused_gnb=1")["fused_gnb"] == 0
    assert ex.parse("fused_gnb=0")["fused_gn"] == 1


@pytest.mark.parametrize("text, item", [
    ("split=0,fuse_skip=0", "fuse_skip=0"),                          # unknown key
    ("split=0,ksplit,split=1", "split=1"),                           # a key given twice
    ("ksplit=on", "ksplit=on"),                                      # not an integer
    ("kpack=", "kpack="),                                            #   "
    ("roll=2", "roll=2"),                                            # a flag other than 0 / 1
    ("fused_head=-1", "fused_head=-1"),                              #   "
    ("wgrad_wgs=0", "wgrad_wgs=0"),                                  # wgrad_wgs < 1
    ("defer_wgrad_levels=-1", "defer_wgrad_levels=-1"),              # defer_wgrad_levels < 0
    ("ablate=wgrad+gn_bwd", "ablate=wgrad+gn_bwd"),                  # unknown ablate member
    ("ablate", "ablate"),                                            #   " (a bare key means =1)
])
def test_parser_refuses(text, item):
    from vdm4cdm_amd import _experiment as ex
    with pytest.raises(ValueError) as err:
        ex.parse(text)
    assert repr(item) in str(err.value) and "valid keys" in str(err.value) and "skip_dgrad_stream" in str(err.value)


# ---- 2. the retired variables -------------------------------------------------------------------
@pytest.mark.parametrize("name, value, new", [("VDM4CDM_NO_SPLIT", "1", "split=0"), ("VDM4CDM_FUSED_SKIP", "0", "fused_skip=0")])
def test_retired_names_are_refused_before_the_library_loads(name, value, new):
    r = child(["-c", "import vdm4cdm_amd._lib"], **{name: value})
    assert r.returncode != 0 and f"{name} is retired" in r.stderr and f"VDM4CDM_EXPERIMENT={new}" in r.stderr, r.stderr[-2000:]


def test_every_retired_name_maps_to_a_key():
    from vdm4cdm_amd import _experiment as ex
    assert len(ex.RETIRED) == 19 and sorted(new.split("=")[0] for new in ex.RETIRED.values()) == sorted(ex.TABLE)
    for new in ex.RETIRED.values():
        ex.parse(new.replace("=N", "=3").replace("=a+b", "=pack"))     # the advice itself is valid


# ---- 3. module constants ------------------------------------------------------------------------
CONSTANTS = ("from vdm4cdm_amd import _experiment, hip_ops, unet_hip, vdm_model\n"
             "print(unet_hip.FUSED_GN, unet_hip.FUSED_GNB, unet_hip.FUSED_SKIP, unet_hip.DEFER_WGRAD_LEVELS)\n"
             "print(vdm_model.FUSED_HEAD, hip_ops.FUSED_TAIL)\n"
             "print(hip_ops.ABLATE)\n"
             "try:\n"
             "    _experiment.refuse_for_training()\n"
             "    print('trains')\n"
             "except RuntimeError as e:\n"
             "    print('refused:', e)\n")


def test_module_constants_follow_the_variable():
    r = child(["-c", CONSTANTS], "fused_gn=0,fused_head=0,defer_wgrad_levels=2,ablate=pack")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[:3] == ["False False True 2", "False True", "{'pack'}"] and lines[3].startswith("refused:") and "pack" in lines[3], r.stdout
    assert "results are WRONG" in r.stderr and "ablate=pack" in r.stderr and "fused_head=0" in r.stderr, r.stderr


def test_module_constants_default_and_banner():
    r = child(["-c", CONSTANTS])
    assert r.returncode == 0 and r.stdout.splitlines() == ["True True True 1", "True True", "set()", "trains"], r.stdout + r.stderr[-2000:]
    assert "VDM4CDM_EXPERIMENT" not in r.stderr                      # nothing differs from the defaults: no banner
    r = child(["-c", CONSTANTS], "ksplit=0, fused_tail=0")           # an A/B switch: announced, usable in training
    assert r.returncode == 0 and r.stdout.splitlines() == ["True True True 1", "True False", "set()", "trains"], r.stdout + r.stderr[-2000:]
    assert "VDM4CDM_EXPERIMENT active: ksplit=0,fused_tail=0" in r.stderr and "WRONG" not in r.stderr, r.stderr
    r = child(["-c", CONSTANTS], "ablate_reduce")
    assert r.returncode == 0 and r.stdout.splitlines()[3].startswith("refused:") and "results are WRONG" in r.stderr, r.stdout + r.stderr


# ---- 4. one table in two languages --------------------------------------------------------------
def test_library_table_equals_the_python_table():
    from vdm4cdm_amd import _experiment as ex
    header = open(os.path.join(CSRC, "experiment.h")).read()
    block = header[header.index("#define VDM_EXPERIMENT_KEYS(X)"):header.index("struct Experiment")]
    rows = [(k, int(d)) for k, d in re.findall(r"\bX\((\w+),\s*(-?\d+)\)", block)]
    assert len(rows) == 10
    assert rows == [(k, d) for k, (d, _, library) in ex.TABLE.items() if library]
    for path in glob.glob(os.path.join(CSRC, "*")):
        if path.endswith((".h", ".hip", "Makefile")):
            read = set(re.findall(r'getenv\("(VDM4CDM_\w*)', open(path).read()))
            assert read <= {"VDM4CDM_EXPERIMENT"}, (path, read)


# ---- 5. the library's parser under AddressSanitizer + UBSan, as a program of its own ------------
def test_library_parser_under_asan_ubsan(tmp_path):
    """Host code only (-x c++: no device code is compiled), and like test_cpu.py::test_host_side_under_asan_ubsan on the CPU container only."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("sanitizer builds are exercised on the CPU container only")
    exe = str(tmp_path / "experiment_parse_check")
    src = os.path.join(ROOT, "tests", "experiment_parse_check.cpp")
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g"] + sanitize + ["-Wall", "-Werror", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "experiment parser ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


# ---- 6. every switch a host query can see still reaches its plans -------------------------------
# roll, grouped_reduce and ablate_reduce change no answer of a host-side query (roll and grouped_reduce choose among launches of the
# same tiles, packed layout and workspace; ablate_reduce skips a launch): the table and parser tests above cover them, and a kernel
# trace on the GPU shows them (conv_roll_kernel with roll; wgrad_reduce_kernel for wgrad_reduce_direct_kernel with grouped_reduce).
THIN = {"in_2_32", "out_32_1"}
REACHES = {
    "kpack=0": THIN,
    "thin_wgrad=0": THIN,
    "split=0": {"c64_16", "c64_8", "c64_32", "c64_32_16"},          # (c64_32: 256 workgroups of 2x8x16 tiles, below two per CU)
    "ksplit=0": {"c128_8", "c128_4", "c256_4", "c256_8"},
    "wgrad_rows=0": None,                                            # None: the eleven that are not THIN
    "wgrad_roll=0": None,
    "wgrad_wgs=256": {"L0_64", "c64_32"},
}


def plan_dump(experiment):
    r = child([os.path.join(ROOT, "tests", "_experiment_plan_dump.py")], experiment)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def default_plans(hip_lib):
    return plan_dump(None)


def test_default_plans_do_not_depend_on_the_spelling(default_plans):
    assert len(default_plans) == 13 and all(len(v) == 31 for v in default_plans.values())
    assert plan_dump("") == default_plans
    assert plan_dump("split=1,ksplit,kpack=1,roll=1,thin_wgrad=1,wgrad_rows=1,wgrad_roll=1,wgrad_wgs=512,grouped_reduce=0,ablate_reduce=0,"
                     "fused_gn=1,ablate=") == default_plans


@pytest.mark.parametrize("setting", sorted(REACHES))
def test_library_switch_reaches_its_plans(default_plans, setting):
    got = plan_dump(setting)
    changed = {k for k in default_plans if got[k] != default_plans[k]}
    assert changed == (REACHES[setting] or set(default_plans) - THIN), f"{setting}: {sorted(changed)}"
