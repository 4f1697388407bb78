"""The noise reference itself (tests/_philox_ref.py) and the case tables of tests/test_step_kernels_gpu.py, checked without a GPU:
published known answers of Philox4x32-10, the three special groups of stream (42, 1), the seed mixing, the partition regimes the shape
tables claim, and - the condition that keeps the GPU checks meaningful - that every emulated fault of FAULTS moves at least one
quantity a GPU check compares, on the very windows and cases of tests/_step_cases.py, by more than 100 times the bound."""
import math

import numpy as np
import pytest

import _philox_ref as P
import _step_cases as S

# Philox4x32-10 known answers (Random123 kat_vectors: zeros; all ones; the digits of pi)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_known_answers():
    for ctr, key, out in KAT:
        got = tuple(int(w) for w in P.philox4x32_10(*ctr, *key))
        assert got == out, (ctr, key, [hex(w) for w in got])
    # vectorised over counters: the three at once
    c = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    k = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = P.philox4x32_10(*c, *k)
    for j, (_, _, out) in enumerate(KAT):
        assert tuple(int(w[j]) for w in got) == out


def test_unit_range():
    assert P.unit(np.array([0, 255], dtype=np.uint32)).tolist() == [2.0 ** -24] * 2
    assert P.unit(np.array([0xFFFFFFFF, 0xFFFFFF00], dtype=np.uint32)).tolist() == [1.0, 1.0]
    assert P.unit(np.array([0x80000000], dtype=np.uint32))[0] == 0.5 + 2.0 ** -24


def test_special_groups_of_stream_a():
    seed, sid = S.STREAM_A
    w = P.stream_words(seed, sid, np.array([S.G_ZERO_23, S.G_ZERO_01, S.G_RMAX], dtype=np.uint64))
    assert int(w[2][0]) >> 8 == 0xFFFFFF and int(w[0][1]) >> 8 == 0xFFFFFF and int(w[0][2]) >> 8 == 0
    x = P.normals(seed, sid, np.array([S.G_ZERO_23, S.G_ZERO_01, S.G_RMAX], dtype=np.uint64))
    assert x[0, 2] == 0.0 and x[0, 3] == 0.0 and x[0, 0] != 0.0          # radius 0: exact zeros
    assert x[1, 0] == 0.0 and x[1, 1] == 0.0 and x[1, 2] != 0.0
    assert math.hypot(x[2, 0], x[2, 1]) == pytest.approx(S.R_MAX, rel=1e-12) and S.R_MAX == pytest.approx(5.768, abs=1e-3)
    # every special group lies inside a window, and inside the field
    for g in (S.G_ZERO_23, S.G_ZERO_01, S.G_RMAX):
        assert any(a <= g < a + c for a, c in S.randn_windows()) and 4 * g + 3 < S.STREAM_A_N
    wins = S.randn_windows()
    assert wins[0] == (0, 4096) and wins[1][0] < S.SWEEP < sum(wins[1]) and wins[-1] == ((S.STREAM_A_N + 3) // 4 - 64, 64)
    assert S.STREAM_A_N % 4 == 3 and all(c > 0 for _, c in wins)


def test_mix_seed():
    assert P.mix_seed(5) == 5 and P.mix_seed(5, 0) == 5                  # step 0 = no counter
    assert P.mix_seed(5, 1) == 5 + P.GOLDEN64
    assert P.mix_seed((1 << 64) - 1, 1) == P.GOLDEN64 - 1                # wraps mod 2^64
    assert P.mix_seed(0, 7) == (7 * P.GOLDEN64) % (1 << 64) and P.mix_seed(0, 7) != 7 * P.GOLDEN64
    assert P.mix_seed(3, -1) == (3 + 0xFFFFFFFF * P.GOLDEN64) % (1 << 64)          # the counter is taken as uint32
    assert P.mix_seed(-((1 << 63) - 11)) == (1 << 63) + 11                         # a seed >= 2^63 handed over as its int64
    for step in (None, 0):
        assert P.time_offset(4242, step) == P.time_offset(4242)
        assert np.array_equal(P.randn(42, 1, 64, step=step), P.randn(42, 1, 64))
    assert not np.array_equal(P.randn(42, 1, 64, step=1), P.randn(42, 1, 64))


def test_consumers_restate_one_stream():
    """The consumer functions differ only in their keying: each is a slice of the randn field of its (seed, stream id)."""
    n, per = 3, 1028
    field = P.randn(11, 5, n * per)
    assert np.array_equal(P.batch_noise(11, 5, n, per), field.reshape(n, per))
    assert np.array_equal(P.ancestral_noise(11, 4, 1030), field[:1030])
    rows = P.ancestral_rows_noise((11, 12), 4, per)
    assert np.array_equal(rows[0], field[:per]) and np.array_equal(rows[1], P.randn(12, 5, per))
    assert np.array_equal(P.randn(11, 5, 40, first_group=7), field[28:68])


@pytest.mark.parametrize("n,per,claim", S.VEC_SHAPES + [S.LOSS_RNG_ONLY], ids=lambda v: None if isinstance(v, dict) else str(v))
def test_vector_shapes_reach_their_regime(n, per, claim):
    r = S.regime(n, per)
    assert per % 4 == 0 and r["rows"] <= S.WS_ROWS
    assert {k: r[k] for k in claim} == claim, r


@pytest.mark.parametrize("n,per,claim", S.SCALAR_SHAPES, ids=lambda v: None if isinstance(v, dict) else str(v))
def test_scalar_shapes_reach_their_regime(n, per, claim):
    r = S.regime(n, per, scalar=True)
    assert per % 4 != 0 and r["rows"] <= S.WS_ROWS, "hip_ops.loss_terms sends per % 4 == 0 to the vector kernel"
    assert {k: r[k] for k in claim} == claim, r


def test_other_tables():
    assert S.VEC_ONCE in [(n, p) for n, p, _ in S.VEC_SHAPES] and S.VEC_SPARSE[0] in [(n, p) for n, p, _ in S.VEC_SHAPES]
    assert S.regime(*S.VEC_TOO_MANY)["rows"] > S.WS_ROWS
    assert S.rows_grid(5, 512_000) == (500, 410) and S.rows_grid(3, 1028) == (2, 2) and S.rows_grid(65535, 4) == (1, 1)
    assert (5, 512_000) in S.ROWS_SHAPES
    n = S.ANCESTRAL_NS[-1]
    grid = S.flat_grid(n, 2048)[1]
    assert grid == 1025 and grid * 256 < (n + 3) // 4 <= 2 * grid * 256 and n % 4 == 2          # two passes, the last group ragged
    assert S.flat_grid(S.PACK_INPUT_NVOX[-1], 256) == (2049, 2048)
    assert S.flat_grid(S.SUMSQ_NS[-1], 4096)[0] > 2048 and S.flat_grid(S.SUMSQ_NS[-2], 4096)[0] == 2049
    assert S.flat_grid(S.STREAM_A_N, 2048)[1] == 2048 and (S.STREAM_A_N + 3) // 4 > 35 * S.SWEEP
    assert S.NORMAL_BOUND == 4 * S.NORMAL_ERR_MEASURED and S.NORMAL_ERR_MEASURED < 2.0 ** -10


# ---- fault coverage ------------------------------------------------------------------------------------------------------------
def _compared(fault):
    """Every quantity a noise check of tests/test_step_kernels_gpu.py compares, as {name: (array, is a field of normals)}."""
    out = {}
    seed, sid = S.STREAM_A
    out["randn A windows"] = (np.concatenate([P.randn(seed, sid, 4 * c, first_group=a, fault=fault) for a, c in S.randn_windows()]), True)
    seed, sid = S.STREAM_B
    out["randn B"] = (P.randn(seed, sid, S.STREAM_B_N, fault=fault), True)
    c = S.PACK_NOISE
    out["diffuse_pack"] = (P.batch_noise(c["seed"], c["sid"], c["n"], c["per"], fault=fault), True)
    c = S.ANCESTRAL_NOISE
    for step in c["steps"]:
        out[f"ancestral step {step}"] = (P.ancestral_noise(c["seed"], step, c["n"], fault=fault), True)
    c = S.ROWS_NOISE
    for step in c["steps"]:
        out[f"ancestral rows step {step}"] = (P.ancestral_rows_noise(c["seeds"], step, c["per"], fault=fault), True)
    V = math.prod(S.MASK_SPATIAL)
    for bf16, c1, c2 in S.MASK_CASES:
        for p in S.MASK_PS:
            for seed in S.MASK_SEEDS:
                out[f"mask bf16={bf16} C={c1}+{c2} p={p} seed={seed}"] = (P.dropout_bytes(seed, p, S.MASK_N, V, c1 + c2, bf16, fault=fault), False)
    for seed in S.TIME_SEEDS:
        out[f"time offset seed={seed}"] = (np.array([P.time_offset(seed, fault=fault)]), False)
    return out


@pytest.fixture(scope="module")
def compared_clean():
    return _compared(None)


@pytest.mark.parametrize("fault", P.FAULTS)
def test_every_fault_is_seen(fault, compared_clean):
    """A check sees the fault when its compared quantity changes: bits for the masks and the time offset; for a field of normals, more
    than half of the elements by more than 100 bounds - then no bound-sized slack can hide it."""
    faulty = _compared(fault)
    seen = []
    for name, (ref, normal) in compared_clean.items():
        got = faulty[name][0]
        if normal:
            frac = float((np.abs(got - ref) > 100 * S.NORMAL_BOUND).mean())
            assert frac == 0.0 or frac > 0.5, f"{fault}: {name} changes only {frac:.3f} of its elements"
            if frac > 0.5:
                seen.append(name)
        elif not np.array_equal(got, ref):
            seen.append(name)
    print(f"{fault}: seen by {len(seen)} of {len(compared_clean)} checks: {seen[:4]}{' ...' if len(seen) > 4 else ''}")
    assert seen, f"no GPU check would notice {fault}"
    if fault not in ("step_not_plus_1", "row_group_batch_flat", "sid_hi_dropped", "seed_hi_dropped"):
        assert "randn A windows" in seen                                  # a generator or transform fault shows in vdm_randn itself


# ---- host fixes: the float4 entries refuse a misaligned field before any launch (no device needed) -------------------------------
def _refused(lib, status, who):
    msg = lib.vdm_last_error().decode()
    assert status == -1 and who in msg and "16-byte aligned" in msg, (status, msg)          # VDM_ERR_ARG


def test_float4_entries_refuse_misaligned_pointers(hip_lib):
    """Pointer VALUES only: the checks return before anything is dereferenced or launched.  Each field in turn sits one float off."""
    A = [0x10000 * (k + 1) for k in range(8)]                              # aligned stand-ins
    a, sg = A[6], A[7]                                                     # alpha / sigma / coef: 4-byte aligned is enough
    for k in range(3):                                                     # x, eps, z_t
        p = [A[j] + (4 if j == k else 0) for j in range(3)]
        _refused(hip_lib, hip_lib.vdm_diffuse(p[0], p[1], a + 4, sg + 4, 2, 1028, p[2], None), "diffuse:")
    for dtype in (0, 1):
        for k in range(5):                                                 # x, s_cond, eps, z_t, packed
            p = [A[j] + (4 if j == k else 0) for j in range(5)]
            _refused(hip_lib, hip_lib.vdm_diffuse_pack(p[0], p[1], p[2], 1, 2, None, a + 4, sg + 4, 2, 1028, dtype, p[3], p[4], None),
                     "diffuse_pack:")
        _refused(hip_lib, hip_lib.vdm_diffuse_pack(A[0] + 8, None, None, 1, 2, None, a, sg, 2, 1028, dtype, None, A[4], None), "diffuse_pack:")
    for k in range(5):                                                     # x, eps, eps_hat, eps0, d_eps_hat
        p = [A[j] + (4 if j == k else 0) for j in range(5)]
        _refused(hip_lib, hip_lib.vdm_loss_terms_rng(p[0], p[1], 1, 2, p[2], p[3], 3, 4, None, 0.5, a + 4, 2, 1028, A[5] + 4, p[4], A[6] + 4, None),
                 "loss_terms_rng:")
    _refused(hip_lib, hip_lib.vdm_loss_terms_rng(A[0], None, 1, 2, A[2] + 12, None, 3, 4, None, 0.5, a, 2, 1028, A[5], A[4], A[6], None),
             "loss_terms_rng:")
