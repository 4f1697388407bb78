"""Shapes, windows and bounds of the noise-source and step-kernel checks (tests/test_noise_cpu.py asserts the regimes on the CPU,
tests/test_step_kernels_gpu.py runs them).  The partition formulas restate the host code of csrc/elementwise.hip:

  vector kernels (diffuse, diffuse_pack, loss_terms_rng): work = per / 4 float4 groups per sample,
      bpn = clamp(ceil(work / 4096), 1, max(1, 2048 // n)) workgroups per sample, thread stride bpn * 256 groups;
  scalar loss_terms: the same with work = per elements;
  the reductions write one partial row per workgroup (bpn * n <= 2048 rows) and fold_partials sums the bpn rows of a sample with 256
  threads: ceil(bpn / 256) passes of the fold loop;
  randn / ancestral_step: min(2048, ceil(n / 2048)) workgroups, a sweep of the full grid is 2048 * 256 = 524 288 groups."""
import math

WS_ROWS = 2048
SWEEP = 2048 * 256                                    # groups one pass of a full randn / ancestral grid covers

# ---- the normal transform's error (3a) -------------------------------------------------------------------------------------------
# Measured on the MI355X: max |device - float64| over the windows below = 1.497e-6 (worst window: the one around G_ZERO_01; the whole
# second stream gives 2.072e-6, the consumers' fields 0.9e-6 to 1.9e-6) - __logf, __sincosf at angles up to 2 pi and the fp32 product
# 2 pi u.  The bound is 4 times the windows' value: they sample the (u0, u1) plane thinly.  A measured value above 2^-10 = 9.8e-4 would be
# a finding about the noise quality; this one is 650 times smaller.
NORMAL_ERR_MEASURED = 1.497e-6
NORMAL_BOUND = 4 * NORMAL_ERR_MEASURED
R_MAX = math.sqrt(48 * math.log(2))                   # sqrt(-2 ln 2^-24) = 5.768: the largest radius

STREAM_A = (42, 1)                                    # (seed, stream id)
STREAM_A_N = 4 * 18_495_200 - 1                       # ragged last group
G_ZERO_23, G_ZERO_01, G_RMAX = 3_640_338, 6_713_667, 18_495_139      # special groups of stream A (found by scanning 2^25 groups)
WINDOW = 4096
STREAM_B = ((1 << 63) + 12345, (1 << 40) + 7)
STREAM_B_N = 1 << 22


def randn_windows():
    """(first group, number of groups) of every window of stream A compared with float64."""
    last = (STREAM_A_N + 3) // 4
    w = [(0, WINDOW), (SWEEP - WINDOW // 2, WINDOW)]
    w += [(g - WINDOW // 2, WINDOW) for g in (G_ZERO_23, G_ZERO_01, G_RMAX)]
    w.append((last - 64, 64))
    return [(a, min(c, last - a)) for a, c in w]


# ---- keying checks (3b, 3c) ------------------------------------------------------------------------------------------------------
# dropout mask cases: (bf16, c1, c2); n = 2, voxels 3 x 5 x 7
MASK_CASES = [(False, 32, 0), (True, 16, 0), (True, 96, 0), (True, 32, 16)]
MASK_N, MASK_SPATIAL = 2, (3, 5, 7)
MASK_PS = (0.1, 0.5)
MASK_SEEDS = (4242, (1 << 40) + 5)
TIME_SEEDS = (3, 4242, (1 << 40) + 5)
SEED_STEPS = (None, 0, 1, 7)                          # the device step counter; None = no counter
PACK_NOISE = dict(seed=(1 << 40) + 12345, sid=3, n=3, per=1028)
ANCESTRAL_NOISE = dict(seed=(1 << 40) + 99, n=1030, steps=(0, 3))
ROWS_NOISE = dict(seeds=(7, (1 << 40) + 7, (1 << 63) + 11), per=1028, steps=(0, 3))


# ---- partition regimes (4) -------------------------------------------------------------------------------------------------------
def regime(n, per, scalar=False):
    work = per if scalar else per // 4
    want = max(1, -(-work // 4096))
    bpn = min(want, max(1, WS_ROWS // n))
    rounds = -(-work // (bpn * 256))
    return dict(work=work, want=want, bpn=bpn, rows=bpn * n, rounds=rounds, last_live=work - (rounds - 1) * bpn * 256,
                fold_passes=-(-bpn // 256))


# (n, per, what the shape is there for: the regime entries test_noise_cpu asserts)
VEC_SHAPES = [
    (1, 4, dict(bpn=1, rounds=1, last_live=1)),                                   # one lane
    (1, 1020, dict(bpn=1, rounds=1, last_live=255)),                              # the 256-thread boundary
    (1, 1024, dict(bpn=1, rounds=1, last_live=256)),
    (1, 1028, dict(bpn=1, rounds=2, last_live=1)),
    (2, 16388, dict(bpn=2, rounds=9, last_live=1)),                               # nine rounds, the last with one live lane
    (2, 49156, dict(bpn=4)),
    (2048, 4, dict(bpn=1, rows=2048)),                                            # every partial row
    (1000, 32772, dict(want=3, bpn=2)),                                           # capped by the sample count
    (1, 4_210_692, dict(bpn=258, rows=258, fold_passes=2)),                       # the fold loop runs twice
]
VEC_ONCE = (1000, 32772)                              # run once per kernel (bf16 for diffuse_pack)
VEC_SPARSE = ((1, 4_210_692), (1, 33_554_440))        # sparse integers: a dense sum would pass 2^24
LOSS_RNG_ONLY = (1, 33_554_440, dict(want=2049, bpn=2048, rows=2048, fold_passes=8))
VEC_TOO_MANY = (2049, 4)                              # no workspace: fine; with workspace: refused
SCALAR_SHAPES = [
    (1, 1, dict(bpn=1, rounds=1, last_live=1)),
    (1, 3, dict(bpn=1, last_live=3)),
    (2, 255, dict(bpn=1, rounds=1, last_live=255)),
    (2, 257, dict(bpn=1, rounds=2, last_live=1)),
    (3, 4097, dict(bpn=2)),
    (2048, 5, dict(bpn=1, rows=2048)),
    (700, 12297, dict(want=4, bpn=2)),
]

# ---- sampler and glue kernels ----------------------------------------------------------------------------------------------------
# the last: 524 290 groups on ceil(n / 2048) = 1025 workgroups (stride 262 400 groups) - every thread but the last few takes two groups,
# the last group holds 2 elements (the size was meant as one sweep of a 2048-workgroup grid plus 2; the grid is sized from n, not capped)
ANCESTRAL_NS = (1, 2, 3, 5, 1023, 2_097_158)
ANCESTRAL_STEPS = (0, 3)                              # rows of a 5-row table
ROWS_SHAPES = [(1, 4), (3, 1028), (5, 512_000), (2049, 4), (65535, 4)]
ROWS_REFUSED = 65536
SUMSQ_NS = (1, 3, 4, 1023, 4097, 8_388_613, 16_777_219)
CLIP_NS = (1, 3, 1023, 4097, 8_388_613)
ELBO_EXACT_B = (1, 2, 64, 2048)
ELBO_REAL_B = (3, 65)
PACK_INPUT_NVOX = (1, 255, 257, 524_291)              # the last exceeds the 2048-workgroup grid


def rows_grid(rows, per):
    """workgroups per row of ancestral_step_rows: (wanted, launched)"""
    want = -(-(per // 4) // 256)
    return want, min(want, -(-2048 // rows))


def flat_grid(n, per_block):
    """workgroups of a grid-stride kernel whose block takes `per_block` elements: (wanted, launched)"""
    want = max(1, -(-n // per_block))
    return want, min(want, 2048)
