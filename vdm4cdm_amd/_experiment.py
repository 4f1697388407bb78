"""The A/B and ablation switches of kernels and streams: one variable, VDM4CDM_EXPERIMENT, a comma-separated list of `key` or `key=value`
items (a bare key means key=1; unset or empty: every default).  Parsed and validated once, here, before the library is loaded
(_lib imports this module); the library reads its own keys from the same variable (csrc/experiment.h, a lenient parser of the same table).

    VDM4CDM_EXPERIMENT=split=0,wgrad_wgs=256 python bench.py ...
    VDM4CDM_EXPERIMENT=ablate=wgrad+conv1    python bench.py ...      (timing only: kernels are skipped, Trainer.fit refuses)
"""
import os
import sys

ENV = "VDM4CDM_EXPERIMENT"
FLAG, COUNT, LIST = "flag", "count", "list"          # 0 / 1; an integer >= its minimum; a `+`-joined subset of ABLATIONS
ABLATIONS = ("conv1", "wgrad", "wgrad1", "gn_fwd", "gn_apply", "pack")

# key: (default, kind, read by the library).  The library rows mirror VDM_EXPERIMENT_KEYS of csrc/experiment.h (tests/test_experiment_cpu.py)
TABLE = {
    "split":              (1, FLAG, True),      # half-chunk workgroups of the NC=4 convs on small grids
    "ksplit":             (1, FLAG, True),      # K-split kernel of the deepest levels
    "kpack":              (1, FLAG, True),      # tap-packed kernel of conv_in / conv_out
    "roll":               (1, FLAG, True),      # rolling-z forward / dgrad kernel at level 0
    "thin_wgrad":         (1, FLAG, True),      # thin-side weight gradient of conv_in / conv_out
    "wgrad_rows":         (1, FLAG, True),      # rows kernel of the full bf16 3^3 stride-1 weight gradients (0: tap-split)
    "wgrad_roll":         (1, FLAG, True),      # rolling z window of the rows kernel
    "wgrad_wgs":          (512, COUNT, True),   # persistent workgroups of a weight-gradient launch
    "grouped_reduce":     (0, FLAG, True),      # grouped slab reduce also for few slabs
    "ablate_reduce":      (0, FLAG, True),      # timing ablation: the slab reduces are NOT launched (wrong gradients)
    "fused_gn":           (1, FLAG, False),     # GroupNorm statistics from the producing conv's epilogue
    "fused_gnb":          (1, FLAG, False),     # GroupNorm backward sums from the producing dgrad conv's epilogue (0 when fused_gn=0)
    "fused_skip":         (1, FLAG, False),     # 1x1x1 skip conv inside norm1's GroupNorm passes
    "fused_tail":         (1, FLAG, False),     # last GroupNorm apply pass folded into conv_in's weight gradient
    "fused_head":         (1, FLAG, False),     # fused head of the training step
    "wgrad_stream":       (1, FLAG, False),     # weight gradients on a side stream
    "skip_dgrad_stream":  (1, FLAG, False),     # skip-path input gradients on a second side stream
    "defer_wgrad_levels": (1, COUNT, False),    # up-path levels whose weight gradients wait for the main stream to move on
    "ablate":             (frozenset(), LIST, False),      # timing ablation: the kernels named are NOT launched (wrong results)
}
COUNT_MIN = {"wgrad_wgs": 1, "defer_wgrad_levels": 0}
WRONG_RESULTS = ("ablate", "ablate_reduce")

# the variables this one replaced: VDM4CDM_<suffix> -> what to write instead
RETIRED = {
    "NO_SPLIT": "split=0", "KSPLIT": "ksplit=0", "NO_KPACK": "kpack=0", "ROLL": "roll=0", "NO_THIN_WGRAD": "thin_wgrad=0",
    "WGRAD_ROWS": "wgrad_rows=0", "WGRAD_ROLL": "wgrad_roll=0", "WGRAD_WGS": "wgrad_wgs=N", "GROUPED_REDUCE": "grouped_reduce",
    "ABLATE_REDUCE": "ablate_reduce", "FUSED_GN": "fused_gn=0", "FUSED_GNB": "fused_gnb=0", "FUSED_SKIP": "fused_skip=0",
    "FUSED_TAIL": "fused_tail=0", "FUSED_HEAD": "fused_head=0", "WGRAD_STREAM": "wgrad_stream=0",
    "SKIP_DGRAD_STREAM": "skip_dgrad_stream=0", "DEFER_WGRAD_LEVELS": "defer_wgrad_levels=N", "ABLATE": "ablate=a+b",
}


def parse(text):
    """`text` (None: unset) -> {key: value} over every key of TABLE; ValueError names the item it refuses."""
    def refuse(item, why):
        return ValueError(f"{ENV}: item {item!r}: {why} (valid keys: {', '.join(TABLE)})")

    out = {k: d for k, (d, _, _) in TABLE.items()}
    seen = set()
    for item in filter(None, (s.strip() for s in (text or "").split(","))):
        key, eq, value = (s.strip() for s in item.partition("="))
        if key not in TABLE:
            raise refuse(item, "unknown key")
        if key in seen:
            raise refuse(item, "key given twice")
        seen.add(key)
        kind = TABLE[key][1]
        if kind == LIST:
            members = frozenset(filter(None, value.split("+"))) if eq else {"1"}
            if not members <= set(ABLATIONS):
                raise refuse(item, f"unknown member {sorted(members - set(ABLATIONS))}, choose from {'+'.join(ABLATIONS)}")
            out[key] = frozenset(members)
            continue
        try:
            v = int(value) if eq else 1
        except ValueError:
            raise refuse(item, "the value is not an integer") from None
        if kind == FLAG and v not in (0, 1):
            raise refuse(item, "a flag takes 0 or 1")
        if kind == COUNT and v < COUNT_MIN[key]:
            raise refuse(item, f"the value must be >= {COUNT_MIN[key]}")
        out[key] = v
    if not out["fused_gn"]:          # the folded backward needs the forward partials for the analytic conditioning-table gradient
        out["fused_gnb"] = 0
    return out


def _from_environment():
    for suffix, new in RETIRED.items():
        if "VDM4CDM_" + suffix in os.environ:
            raise RuntimeError(f"VDM4CDM_{suffix} is retired: use {ENV}={new}")
    active = parse(os.environ.get(ENV))
    changed = {k: v for k, v in active.items() if v != TABLE[k][0]}
    if changed:
        shown = ",".join(f"{k}={'+'.join(sorted(v)) if TABLE[k][1] == LIST else v}" for k, v in changed.items())
        if any(k in changed for k in WRONG_RESULTS):
            print(f"\n*** vdm4cdm_amd: {ENV}={shown} - kernels are SKIPPED and results are WRONG "
                  "(timing ablations of tools/ablate_step.sh only; Trainer.fit refuses to run) ***\n", file=sys.stderr, flush=True)
        else:
            print(f"vdm4cdm_amd: {ENV} active: {shown}", file=sys.stderr, flush=True)
    return active


_ACTIVE = _from_environment()


def get(key):
    return _ACTIVE[key]


def refuse_for_training():
    """The timing ablations skip kernels: never train with them (Trainer.fit)."""
    if get("ablate") or get("ablate_reduce"):
        raise RuntimeError(f"{ENV}: ablate={sorted(get('ablate'))} ablate_reduce={get('ablate_reduce')} is set: "
                           "kernels are skipped and gradients are garbage - unset it")
