"""Case table and operands of the K6 parity tests (csrc/cond.hip: the conditioning MLPs and the additive injection table; device half
tests/test_cond_kernels_gpu.py, host half tests/test_cond_cpu.py, reference and bounds tests/_cond_ref.py).

Every case names the code edge it is there for (`edge`) and the properties that put it on that edge (`expect`), which
tests/test_cond_cpu.py recomputes from the constants of cond.hip restated below (`props`)."""
import math
from collections import namedtuple

import torch

# ---- constants of csrc/cond.hip, restated (not imported from the product) -----------------------------------------------------------
COND_MAX = 4                # conditionings per call
COND_MAXDIM = 256           # widest hidden layer / input
FSLAB = 64                  # table columns per forward workgroup
BSLAB = 32                  # table columns per backward slab
QUADS_PER_PASS = 8          # dot_row: 16-byte loads in flight per thread and pass
FOLD_PER_PASS = 8           # backward: strided loads in flight per thread and pass (slab rows, slab partials, rows of W2)
PARAM_BLOCKS, THREADS = 2048, 256         # cond_table_bwd_params_kernel: grid cap, block size
STEP_BLOCKS = 64            # cond_table_step_kernel: grid cap
MAX_ROWS = 65535
LN_1E4 = 9.210340371976184  # the constant of the frequency law 10000^(-i / half)


def tpo_for(dim):
    """threads per output of the MLP layers; also the row-groups (nws) of the backward kernels"""
    return 4 if dim <= 64 else (2 if dim <= 128 else 1)


# ---- library errors, measured on an MI355X (test_cond_kernels_gpu.py::test_library_errors prints them) --------------------------------
# In units of u |result|, u = 2^-24 (one ulp of the result is between u and 2u of it).  Each constant is 4 times the measured maximum,
# the margin of _step_cases.NORMAL_BOUND: a maximum over 10^4 draws understates the tail.
#   erff: through the (h2, c) pairs of `saved`, c = gelu_f(h2) against float64 at the device's own h2, ALL of the error of gelu_f charged
#         to erff: |c - gelu64(h2)| * 2 / |h2| / (u |erf(h2 / sqrt 2)|) over the pairs with 0.5 <= |h2| <= 6 (below 0.5 the rounding of
#         1 + erf, which the bound carries on its own, is all there is to see: K_ERF is ASSUMED there, not measured; the test holds the
#         whole model E_gelu against the device over all of |h2| <= 6 instead).
#   sinf / cosf: through the saved embedding at i = 0 (f = 1) and t = m 2^-14, m = 0..16383: the argument 1000 t is exact in fp32.
#   f = expf(-ln 1e4 * i / half): through the saved sin(1000 t f_i) at t = 2^-20, where sin(a) = a (1 - a^2 / 6) to 1e-13: the relative
#         error of the device's f against float64, all (i, half) with half = 1..128; it holds the two roundings of the argument
#         (about 2 * 9.21 u), expf's own error and one rounding each of the product 1000 t f and of sinf at a tiny argument.
ERF_ERR_MEASURED = 5.418          # = 4.434 ulp of erf, 12607 pairs
SINCOS_ERR_MEASURED = 1.932       # = 1.460 ulp of the result, 32768 values
FREQ_ERR_MEASURED = 20.257        # 8256 (i, half) pairs; 2 * 9.21 u of it are the argument's two roundings
K_ERF = 4 * ERF_ERR_MEASURED
K_SINCOS = 4 * SINCOS_ERR_MEASURED
K_FREQ = 4 * FREQ_ERR_MEASURED
FINDING_ULP = 8.0           # a measured erff / sinf / cosf error above 8 ulp of the result is a finding, not a constant

Mlp = namedtuple("Mlp", "sinusoid in_dim dim")
Case = namedtuple("Case", "name mlps rows width edge expect")


def t(in_dim, dim):
    return Mlp(True, in_dim, dim)


def v(in_dim, dim):
    return Mlp(False, in_dim, dim)


CASES = [
    Case("v1_3", [v(1, 3)], 2, 1,
         "every dot product is scalar tail only; one table column; one backward slab of one column",
         dict(quads=[(0, 0)], fslabs=1, bslabs=1, last_bslab=1, last_fslab=1)),
    Case("v3_65", [v(3, 65)], 5, 33,
         "tpo = 2 with odd lengths; the backward's second slab holds one column",
         dict(tpo=[2], quads=[(0, 0)], bslabs=2, last_bslab=1)),
    Case("v6_64", [v(6, 64)], 7, 65,
         "tpo = 4; the forward's second slab holds one column",
         dict(tpo=[4], fslabs=2, last_fslab=1)),
    Case("v4_128", [v(4, 128)], 3, 129,
         "tpo = 2; the 16-byte path of the dim-long dot products takes two full passes (the in_dim-long one a single quad)",
         dict(tpo=[2], quads=[(1, 32)], passes=[(1, 2)], partial_pass=[(True, False)])),
    Case("v252_132", [v(252, 132)], 2, 300,
         "tpo = 1; 33 quads, the last pass partial; nws = 1, 10 slabs: a second fold pass in the rows kernel",
         dict(tpo=[1], quads=[(63, 33)], passes=[(8, 5)], partial_pass=[(True, True)], bslabs=10, fold_passes=[2])),
    Case("v256_256", [v(256, 256)], 3, 2080,
         "more than 2048 * 256 parameter-gradient elements: the params kernel's grid-stride loop takes a second trip; 65 slabs",
         dict(tpo=[1], param_trips=2, bslabs=65)),
    Case("t64_64_v6_64", [t(64, 64), v(6, 64)], 4, 1056,
         "33 slabs at nws = 4: a second fold pass; the shape class of the real network",
         dict(tpo=[4, 4], bslabs=33, fold_passes=[2, 2])),
    Case("four_mlps", [t(2, 3), v(5, 65), v(64, 128), v(256, 256)], 3, 97,
         "COND_MAX conditionings; tpo 4, 2, 2, 1; saved, scratch and partial offsets of uneven sizes; half = 1",
         dict(n=COND_MAX, tpo=[4, 2, 2, 1], half=[1, None, None, None], uneven=True)),
    Case("t256_64", [t(256, 64)], 1, 64,
         "the widest embedding; a single row; exactly one full slab forward",
         dict(half=[128], fslabs=1, last_fslab=64, bslabs=2, last_bslab=32)),
    Case("t6_16", [t(6, 16)], 9, 31,
         "half = 3: the sinusoid width even but no multiple of 4",
         dict(half=[3], quads=[(0, 4)])),
]
CASE_IDS = [c.name for c in CASES]


def cdiv(a, b):
    return (a + b - 1) // b


def quads(length):
    """16-byte loads of one dot product of `length`: the vector path exists only when length % 4 == 0"""
    return length // 4 if length % 4 == 0 else 0


def chain(length, tpo):
    """fused multiply-adds the busiest of the `tpo` lanes of dot_row passes: its quads (4 each), then its share of the scalar tail"""
    nq = quads(length)
    return 4 * cdiv(nq, tpo) + cdiv(length - 4 * nq, tpo)


def saved_floats(case):
    return sum(case.rows * (m.in_dim + 3 * m.dim) for m in case.mlps)


def scratch_floats(case):
    return sum(case.rows * (2 + cdiv(case.width, BSLAB)) * m.dim for m in case.mlps)


def param_total(case, dbias=True):
    return sum(m.dim * m.in_dim + m.dim + m.dim * m.dim + m.dim + case.width * m.dim for m in case.mlps) + (case.width if dbias else 0)


def props(case):
    """The path-deciding quantities of a case, computed from the restated constants."""
    ms = case.mlps
    bslabs = cdiv(case.width, BSLAB)
    p = dict(n=len(ms), tpo=[tpo_for(m.dim) for m in ms], quads=[(quads(m.in_dim), quads(m.dim)) for m in ms],
             half=[m.in_dim // 2 if m.sinusoid else None for m in ms],
             fslabs=cdiv(case.width, FSLAB), last_fslab=case.width - (cdiv(case.width, FSLAB) - 1) * FSLAB,
             bslabs=bslabs, last_bslab=case.width - (bslabs - 1) * BSLAB,
             fold_passes=[cdiv(bslabs, FOLD_PER_PASS * tpo_for(m.dim)) for m in ms],
             param_trips=cdiv(param_total(case), PARAM_BLOCKS * THREADS))
    p["passes"] = [tuple(cdiv(q, QUADS_PER_PASS * tp) for q in qs) for qs, tp in zip(p["quads"], p["tpo"])]
    p["partial_pass"] = [tuple(q % (QUADS_PER_PASS * tp) != 0 for q in qs) for qs, tp in zip(p["quads"], p["tpo"])]
    p["uneven"] = len({m.in_dim + 3 * m.dim for m in ms}) == len(ms) and len({m.dim for m in ms}) == len(ms)
    return p


# ---- operands -------------------------------------------------------------------------------------------------------------------------
# One dict per case: rows, width, dtable [rows, width], mlps = list of dicts {sinusoid, in_dim, dim, input ([rows] for t, [rows, in_dim]
# for a vector), w1 [dim, in_dim], b1, w2 [dim, dim], b2, wproj [width, dim]}, all fp32 on the CPU.
NNZ = 16                    # nonzeros per row of w1 / w2 in check A: h1 and h2 still hit 0 in 2 - 15 % of the elements
NNZ_PROJ = 256              # wproj is dense in check A: it feeds no pre-activation (largest sum of magnitudes 324 416 < 2^22)
K6I_T_VALUES = [1.0, 0.0, 1e-4, 0.5]          # as tests/test_input_grad_kernels_gpu.py: the ends of the range, where sin / cos saturate


def _sparse(rows, length, nnz, scale, g):
    """[rows, length] with min(length, nnz) entries of +-scale per row; the runs walk a random permutation of the columns so that every
    column carries a nonzero once rows * nnz >= length."""
    nnz = min(length, nnz)
    perm = torch.randperm(length, generator=g)
    cols = perm[(torch.arange(rows)[:, None] * nnz + torch.arange(nnz)[None, :]) % length]
    sign = torch.randint(0, 2, (rows, nnz), generator=g).float() * 2 - 1
    return torch.zeros(rows, length).scatter_(1, cols, sign * scale)


def _small(shape, g, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def ops_a_seed(case, seed):
    g = torch.Generator().manual_seed(seed)
    mlps = []
    for m in case.mlps:
        inp = torch.zeros(case.rows) if m.sinusoid else _small((case.rows, m.in_dim), g)
        mlps.append(dict(sinusoid=m.sinusoid, in_dim=m.in_dim, dim=m.dim, input=inp,
                         w1=_sparse(m.dim, m.in_dim, NNZ, 16.0, g), b1=16.0 * _small((m.dim,), g),
                         w2=_sparse(m.dim, m.dim, NNZ, 1.0, g), b2=16.0 * _small((m.dim,), g),
                         wproj=_sparse(case.width, m.dim, NNZ_PROJ, 1.0, g)))
    return dict(rows=case.rows, width=case.width, mlps=mlps, dtable=_small((case.rows, case.width), g))


def ops_a(case, accept):
    """Check A's operands: the first seed (from a base fixed per case) whose operands `accept` (the four conditions of check A, which
    _cond_ref.ref_int evaluates); the tiny case needs a few draws before h1 and h2 each show all three signs and the backward half is live."""
    base = 1000 * (CASE_IDS.index(case.name) + 1)
    for seed in range(base, base + 200):
        ops = ops_a_seed(case, seed)
        if accept(ops):
            return ops
    raise AssertionError(f"{case.name}: no seed in {base}..{base + 199} satisfies the conditions of check A")


def ops_b(case, seed=7):
    """Check B's operands: random reals in the scale of the network's initialisation; t takes K6I_T_VALUES, then uniform draws."""
    g = torch.Generator().manual_seed(seed + 100 * (CASE_IDS.index(case.name) if case.name in CASE_IDS else len(CASE_IDS)))

    def uni(shape, fan):
        return (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan)

    mlps = []
    for m in case.mlps:
        if m.sinusoid:
            tv = torch.cat([torch.tensor(K6I_T_VALUES), torch.rand(max(case.rows - len(K6I_T_VALUES), 0), generator=g)])[:case.rows]
            inp = tv.float().contiguous()
        else:
            inp = torch.randn(case.rows, m.in_dim, generator=g)
        mlps.append(dict(sinusoid=m.sinusoid, in_dim=m.in_dim, dim=m.dim, input=inp,
                         w1=uni((m.dim, m.in_dim), m.in_dim), b1=uni((m.dim,), m.in_dim),
                         w2=uni((m.dim, m.dim), m.dim), b2=uni((m.dim,), m.dim),
                         wproj=uni((case.width, m.dim), m.dim)))
    return dict(rows=case.rows, width=case.width, mlps=mlps, dtable=torch.randn(case.rows, case.width, generator=g))
