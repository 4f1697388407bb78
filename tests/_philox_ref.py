"""Independent numpy reference of the noise source (tests/test_noise_cpu.py, tests/test_step_kernels_gpu.py).

Philox4x32-10 is written from the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11):
a round replaces the counter (c0, c1, c2, c3) by (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped by
the Weyl constants between rounds.  Everything a consumer of the stream does with the words is restated here, one function per consumer:

  consumer                     key                    counter (c0, c1, c2, c3)              use of the four words
  randn(seed, sid)             mix_seed(seed, step)   (g lo, g hi, sid lo, sid hi)          4 normals = elements 4g .. 4g+3; g = flat group
  diffuse_pack / loss_terms_rng  "                    g = n * per/4 + i: the batch's flat group, i.e. the randn field of shape (n, per)
  ancestral_step(seed, step)   seed                   (g lo, g hi, step + 1, 0)             g = flat group of the whole z
  ancestral_step_rows          seeds[r]               (g lo, g hi, step + 1, 0)             g = group inside row r
  dropout keep byte            mix_seed(seed, step)   (piece lo, piece hi, 0x5eed, 0)       bit j of the byte: element j of the piece
  train_scalars offset         mix_seed(seed, step)   (0, 0, 0x71e5, 0)                     unit(word 0)

  unit(u) = ((u >> 8) + 1) 2^-24 in (0, 1];  normals: words (0, 1) -> r cos t, r sin t with r = sqrt(-2 ln unit(w0)), t = 2 pi unit(w1);
  words (2, 3) -> elements 2, 3 the same way.  mix_seed(seed, step) = (seed + uint32(step) * 0x9E3779B97F4A7C15) mod 2^64.

FAULTS names the emulated faults: every function takes `fault=` and then computes what a kernel with that fault would; the CPU test
asserts that each of them moves at least one quantity the GPU checks compare, by far more than the checks' bound."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # Weyl key increments (golden ratio, sqrt(3) - 1)
GOLDEN64 = 0x9E3779B97F4A7C15
MASK32, MASK64 = 0xFFFFFFFF, (1 << 64) - 1
SID_DROPOUT, SID_TIME = 0x5EED, 0x71E5

FAULTS = ["rounds_9", "multipliers_swapped", "key_not_bumped", "idx_sid_exchanged", "seed_hi_dropped", "sid_hi_dropped",
          "word_pairs_exchanged", "sin_cos_exchanged", "shift_9", "step_not_plus_1", "row_group_batch_flat"]


def _u64(a):
    """Python ints (negative = the int64 image of a value >= 2^63) and integer arrays as uint64."""
    if isinstance(a, int):
        return np.uint64(a & MASK64)
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1, fault=None):
    """Four uint32 words per counter; every argument a 32-bit value or an array of them (broadcast together)."""
    assert fault is None or fault in FAULTS, fault
    mask = np.uint64(MASK32)
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(a) & mask for a in (c0, c1, c2, c3, k0, k1)))
    m0, m1 = (M1, M0) if fault == "multipliers_swapped" else (M0, M1)
    for _ in range(9 if fault == "rounds_9" else 10):
        p0, p1 = np.uint64(m0) * c0, np.uint64(m1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
        if fault != "key_not_bumped":
            k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def unit(u, fault=None):
    """uint32 -> (0, 1] on the 2^-24 grid, float64 (exact; the same value in float32)."""
    return ((_u64(u) >> np.uint64(9 if fault == "shift_9" else 8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24


def mix_seed(seed, step=None):
    """The key of a draw under the device step counter; None = no counter."""
    seed = int(seed) & MASK64
    return seed if step is None else (seed + (int(step) & MASK32) * GOLDEN64) & MASK64


def stream_words(seed, sid, idx, fault=None):
    """The four words of counter `idx` (array) of stream (seed, sid) - the keying every consumer shares.  seed and sid may be arrays
    too (broadcast against idx)."""
    seed, sid, idx = _u64(seed), _u64(sid), _u64(idx)
    lo, hi = (lambda v: v & np.uint64(MASK32)), (lambda v: v >> np.uint64(32))
    i_lo, i_hi = lo(idx), hi(idx)
    s_lo, s_hi = lo(sid), (0 if fault == "sid_hi_dropped" else hi(sid))
    k_lo, k_hi = lo(seed), (0 if fault == "seed_hi_dropped" else hi(seed))
    if fault == "idx_sid_exchanged":
        w = philox4x32_10(s_lo, s_hi, i_lo, i_hi, k_lo, k_hi, fault)
    else:
        w = philox4x32_10(i_lo, i_hi, s_lo, s_hi, k_lo, k_hi, fault)
    return (w[2], w[3], w[0], w[1]) if fault == "word_pairs_exchanged" else w


def _box_muller(w0, w1, fault):
    r = np.sqrt(-2.0 * np.log(unit(w0, fault)))
    t = 2.0 * np.pi * unit(w1, fault)
    return (r * np.sin(t), r * np.cos(t)) if fault == "sin_cos_exchanged" else (r * np.cos(t), r * np.sin(t))


def normals(seed, sid, groups, fault=None):
    """float64 [len(groups), 4]: the four normals of each element group of stream (seed, sid)."""
    w = stream_words(seed, sid, groups, fault)
    a, b = _box_muller(w[0], w[1], fault)
    c, d = _box_muller(w[2], w[3], fault)
    return np.stack([a, b, c, d], axis=-1)


# ---- one function per consumer --------------------------------------------------------------------------------------------------
def randn(seed, sid, n, step=None, first_group=0, fault=None):
    """Elements [4 first_group, 4 first_group + n) of the field vdm_randn(seed, sid) writes (float64)."""
    groups = np.arange(first_group, first_group + (n + 3) // 4, dtype=np.uint64)
    return normals(mix_seed(seed, step), sid, groups, fault).reshape(-1)[:n]


def batch_noise(seed, sid, n, per, step=None, fault=None):
    """diffuse_pack / loss_terms_rng: sample s, group i of the sample = group s * per/4 + i of the stream; [n, per]."""
    assert per % 4 == 0
    return randn(seed, sid, n * per, step, fault=fault).reshape(n, per)


def ancestral_noise(seed, step, n, fault=None):
    """ancestral_step at table row `step`: stream id step + 1, flat groups of z."""
    return randn(seed, step if fault == "step_not_plus_1" else step + 1, n, fault=fault)


def ancestral_rows_noise(seeds, step, per, fault=None):
    """ancestral_step_rows: row r restarts at group 0 of its own seed; [rows, per]."""
    assert per % 4 == 0
    sid = step if fault == "step_not_plus_1" else step + 1
    seeds = np.array([int(s) & MASK64 for s in seeds], dtype=np.uint64) if isinstance(seeds, (tuple, list)) else _u64(seeds)
    groups = np.arange(per // 4, dtype=np.uint64)[None, :] + np.zeros((len(seeds), 1), dtype=np.uint64)
    if fault == "row_group_batch_flat":
        groups = groups + (np.arange(len(seeds), dtype=np.uint64) * np.uint64(per // 4))[:, None]
    return normals(seeds[:, None], sid, groups, fault).reshape(len(seeds), per)


def dropout_bytes(seed, p, n, voxels, channels, bf16, step=None, fault=None):
    """uint8 [n, voxels, channels / EPL]: the keep byte of every 16-byte piece (EPL = 8 bf16 or 4 fp32 elements); bit j set = element j
    of the piece is kept.  piece = n V C/EPL + v C/EPL + column."""
    ppv = channels // (8 if bf16 else 4)
    assert ppv * (8 if bf16 else 4) == channels
    w = stream_words(mix_seed(seed, step), SID_DROPOUT, np.arange(n * voxels * ppv, dtype=np.uint64), fault)
    p32 = np.float32(p)
    out = np.zeros(n * voxels * ppv, dtype=np.uint8)
    if bf16:
        thr = np.uint32(np.float32(p32 * np.float32(65536.0)) + np.float32(0.5))
        for j in range(8):
            field = (w[j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xFFFF)
            out |= (field >= thr).astype(np.uint8) << np.uint8(j)
    else:
        for j in range(4):
            out |= (unit(w[j], fault) > np.float64(p32)).astype(np.uint8) << np.uint8(j)
    return out.reshape(n, voxels, ppv)


def time_offset(seed, step=None, fault=None):
    """train_scalars without u0 and times: the one uniform draw of the step (float64; 1.0 wraps to t = 0 in the kernel)."""
    w = stream_words(mix_seed(seed, step), SID_TIME, np.zeros(1, dtype=np.uint64), fault)
    return float(unit(w[0], fault)[0])
