"""Shapes and cases of the multistep-sampler tests (test_multistep_cpu.py, test_multistep_kernels_gpu.py,
test_multistep_sampler_gpu.py)."""
from _step_cases import ANCESTRAL_NS, ANCESTRAL_STEPS

# ---- tables ----------------------------------------------------------------------------------------------------------------------
TABLE_NS = (1, 2, 3, 10)
TABLE_RTOL, TABLE_ATOL = 1e-12, 1e-15                 # the project's own for step_table (tests/test_cpu.py)
CONVERGENCE_NS = (64, 128, 256, 512)
PRIOR_STDS = (0.5, 2.0)
SECOND_ORDER_RATIO = (3.5, 4.5)                       # error ratio per doubling of n
FIRST_ORDER_RATIO = (1.8, 2.2)

# ---- kernel ----------------------------------------------------------------------------------------------------------------------
# 1, 2, 3: tail only; 5: one float4 group and a tail of one; 1023: 255 groups + 3; the last: more groups than one sweep of its grid
# (1025 workgroups) and a tail of two
KERNEL_NS = ANCESTRAL_NS
KERNEL_ROWS = ANCESTRAL_STEPS                         # rows 0 (w_p == 0) and 3 (w_p != 0) of a 5-row table
KERNEL_TABLE_ROWS = 5
# exact case: every product and sum below is an integer or a dyadic rational far inside 2^24 (fields in [-8, 8], |w_cfg blend| <= 20,
# |est| <= 2 * 8 + 2 * 20 = 56, |z'| <= 4 * 8 + 4 * 56 + 2 * 56 = 368), so fp32 computes it exactly however it is contracted
EXACT_ROW_FIRST = (2.0, -2.0, 0.5, 4.0, 0.0)          # e_z, e_e, w_z, w_x, w_p
EXACT_ROW_SECOND = (1.0, -2.0, 4.0, 3.0, -2.0)
EXACT_W_CFG = 0.5                                     # 1 + w = 1.5: (1 + w) eh - w eu is exact for even-integer fields
SENTINEL = 12345.0
PAD = 8                                               # elements past n that must stay untouched

# ---- sampler ---------------------------------------------------------------------------------------------------------------------
NET_CFG = dict(D=16, chs=(16, 32, 64), sc=1, vd=(6,), pm="zeros")      # CFGS[0] of tests/test_unet_gpu.py
GRAPH_STEPS = 12
ORACLE_STEPS = 20
CFG_STEPS, W_CFG = 12, 0.7
ROW_SEEDS = [1_000_020, 123_456_789_012, 3]           # SEEDS[1], [3], [4] of tests/test_batched_sampling_gpu.py
ENTRY_STEPS, ENTRY_REP = 4, 3


def sampler_tolerance(ref_abs_max):
    """2e-5 max|ref| + 1e-3: the project's own sampler tolerance (test_sampler_matches_oracle)."""
    return 2e-5 * ref_abs_max + 1e-3
