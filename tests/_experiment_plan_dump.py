"""Child process of tests/test_experiment_cpu.py: what the host-side plan queries of the library answer for 13 bf16 descriptors under
the VDM4CDM_EXPERIMENT of this process, as one JSON object {id: [answers]} on stdout.  (A process of its own per setting: the library
reads the variable once.)"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vdm4cdm_amd import _lib  # noqa: E402

# id: n, (od, oh, ow), cin, cout, out_f32 - all ksize 3, stride 1, zero padding, bf16
DESCRIPTORS = {
    "in_2_32": (2, (32, 32, 32), 2, 32, 0),
    "L0_32": (2, (32, 32, 32), 32, 32, 0),
    "L0_16": (2, (16, 16, 16), 32, 32, 0),
    "L0_64": (2, (64, 64, 64), 32, 32, 0),
    "out_32_1": (2, (32, 32, 32), 32, 1, 1),
    "c64_16": (2, (16, 16, 16), 64, 64, 0),
    "c64_8": (1, (8, 8, 8), 64, 64, 0),
    "c64_32": (2, (32, 32, 32), 64, 64, 0),
    "c128_8": (2, (8, 8, 8), 128, 128, 0),
    "c128_4": (1, (4, 4, 16), 128, 128, 0),
    "c256_4": (2, (4, 4, 16), 256, 256, 0),
    "c256_8": (2, (8, 8, 16), 256, 256, 0),
    "c64_32_16": (1, (16, 16, 16), 64, 32, 0),
}


def answers(L, d):
    out = [L.vdm_conv_kernel_variant(d, g) for g in (0, 1)] + [L.vdm_conv_packed_bytes(d, g) for g in (0, 1)]
    out += [L.vdm_conv_gn_tiles(d), L.vdm_conv_dgrad_gn_tiles(d), L.vdm_conv_wgrad_workspace_bytes(d)]
    for want_bias, accumulate in ((0, 0), (1, 0), (0, 1)):
        info = _lib.WgradPlanInfo()
        out.append(L.vdm_conv_wgrad_plan(d, want_bias, accumulate, C.byref(info)))
        out += [getattr(info, k) for k, _ in _lib.WgradPlanInfo._fields_]
    return out


if __name__ == "__main__":
    L = _lib.lib()
    print(json.dumps({k: answers(L, _lib.ConvDesc(n=n, od=od, oh=oh, ow=ow, cin=cin, cout=cout, ksize=3, stride=1, upsample=0, pad_mode=0,
                                                  dtype=_lib.VDM_BF16, out_f32=f32))
                      for k, (n, (od, oh, ow), cin, cout, f32) in DESCRIPTORS.items()}))
