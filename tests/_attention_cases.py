"""Case table and operands of the attention kernel checks (tests/test_attention_cpu.py, tests/test_attention_kernels_gpu.py).  No device
use: everything here is fp32 on the CPU, already rounded to the storage type of the run, in the layouts the kernels read -
q, k, v [N, H, V, hd], dO / out [N, V, H * hd], lse / dsum [N, H, V]."""
import torch

from _exact import ints

# (N, H, V, hd).  The fp32 key tile is 16 wide, the bf16 one 32 (two 16-key sub-tiles), a workgroup is 4 waves of 16 queries / keys.
CASES = [
    (1, 1, 4, 16),         # one 4-key group: every other lane of the tile is clamped to column 0
    (1, 2, 8, 32), (1, 2, 12, 32),
    (2, 1, 20, 16),        # fp32: one full tile + 4 keys; bf16: less than one tile
    (1, 2, 24, 16), (2, 1, 28, 64),
    (1, 3, 36, 128),       # bf16: one tile + 4 keys
    (1, 1, 40, 16), (2, 2, 44, 96), (1, 1, 48, 32), (1, 1, 52, 16), (1, 2, 60, 32),
    (1, 1, 64, 16),        # exactly one workgroup, no ragged tile in either dtype
    (1, 1, 68, 64),        # a second workgroup whose only live wave has 4 live queries
    (2, 3, 132, 32),       # samples x heads (the isolation case)
    (2, 1, 100, 128), (1, 1, 216, 96),
    (1, 1, 256, 16),       # power of two: the uniform forward is exact
    (1, 2, 1028, 64),      # many tiles, 17 workgroups
]
ISOLATION_CASE = (2, 3, 132, 32)
ROWDOT_GRID_STRIDE = (1, 1, 2 ** 20 + 16, 16)          # N V H > 4096 x 256: the grid-stride loop of attn_rowdot_kernel takes a second turn
HEAD_WIDTHS = (16, 32, 64, 96, 128)
ONEHOT_SCALE = 64.0
DTYPES = ["f32", "bf16"]
IDS = [f"n{n}_h{h}_v{v}_hd{hd}" for n, h, v, hd in CASES]


def coverage_gaps(cases):
    """What the issue asks of the table; returns the list of unmet requirements (empty = covered)."""
    gaps = []
    vs = [v for _, _, v, _ in cases]
    for r in range(0, 32, 4):
        if not any(v % 32 == r for v in vs):
            gaps.append(f"no V with V mod 32 == {r}")
    for what, ok in (("a V = 4", 4 in vs), ("two V below 16", sum(v < 16 for v in vs) >= 2), ("two V in 16..32", sum(16 <= v <= 32 for v in vs) >= 2),
                     ("V = 64", 64 in vs), ("V = 68", 68 in vs), ("V = 256", 256 in vs), ("a V >= 1024", any(v >= 1024 for v in vs)),
                     ("a V > 128 with N = 2 and H >= 2", any(v > 128 and n == 2 and h >= 2 for n, h, v, _ in cases))):
        if not ok:
            gaps.append("no " + what)
    for hd in HEAD_WIDTHS:
        rows = [(n, h) for n, h, _, w in cases if w == hd]
        if len(rows) < 2:
            gaps.append(f"head width {hd} appears {len(rows)} times")
        if not any(h > 1 for _, h in rows):
            gaps.append(f"head width {hd} never with H > 1")
        if not any(n > 1 for n, _ in rows):
            gaps.append(f"head width {hd} never with N > 1")
    if any(v % 4 or v < 4 for v in vs) or any(hd not in HEAD_WIDTHS for *_, hd in cases):
        gaps.append("a case the kernels refuse")
    return gaps


def storage(t, bf16):
    """Round to the storage type (nearest even), kept as fp32."""
    return t.float().bfloat16().float() if bf16 else t.float()


def to_heads(x, H):
    """[N, V, H * hd] -> [N, H, V, hd]"""
    N, V, C = x.shape
    return x.reshape(N, V, H, C // H).permute(0, 2, 1, 3).contiguous()


def _gen(case, seed):
    n, h, v, hd = case
    return torch.Generator().manual_seed(seed * 1000003 + ((n * 7 + h) * 4099 + v) * 131 + hd)


def onehot_qk(case, seed=1):
    """k: V distinct rows of +-1 per (sample, head), drawn without replacement (the low 16 entries are the bits of V different numbers
    below 2^16, the other entries are free); q_i = k[pi(i)] with pi a random map that is no bijection, pi(0) = V - 1 and pi(V - 1) = 0.
    With scale = 64 the matching score is 64 hd and every other one at most 64 (hd - 2): exp of the difference is 0 in fp32 and P is
    one-hot.  Returns (q, k [N, H, V, hd], pi [N, H, V] int64)."""
    N, H, V, hd = case
    g = _gen(case, seed)
    k = torch.empty(N, H, V, hd)
    pi = torch.empty(N, H, V, dtype=torch.int64)
    for n in range(N):
        for h in range(H):
            low = torch.randperm(2 ** 16, generator=g)[:V]
            bits = (low[:, None] >> torch.arange(16)[None]) & 1
            rest = torch.randint(0, 2, (V, hd - 16), generator=g)
            k[n, h] = torch.cat([bits, rest], 1).float() * 2 - 1
            p = torch.randint(0, V, (V,), generator=g)
            p[0], p[V - 1] = V - 1, 0
            if p.unique().numel() == V:
                p[2] = p[1]
            pi[n, h] = p
    assert all(k[n, h].unique(dim=0).shape[0] == V for n in range(N) for h in range(H))
    q = torch.gather(k, 2, pi[..., None].expand(N, H, V, hd))
    return q, k, pi


def real_values(case, seed, bf16, shape=None):
    """Random reals rounded to the storage type."""
    N, H, V, hd = case
    return storage(torch.randn(shape or (N, H, V, hd), generator=_gen(case, seed)), bf16)


def int_values(case, seed, r=2, shape=None, terms=None):
    """Integers in {-r..r} as fp32 (exact in bf16 too); r = 2 is _exact.ints, which also checks that a sum of `terms` products (default:
    V, a column sum over the keys) stays below 2^24."""
    N, H, V, hd = case
    shape = shape or (N, H, V, hd)
    if r == 2:
        return ints(shape, _gen(case, seed).initial_seed() % (2 ** 31), terms or V)
    return torch.randint(-r, r + 1, shape, generator=_gen(case, seed)).float()


def onehot_backward_operands(case, bf16):
    """dO [N, V, H hd], v [N, H, V, hd] and dsum [N, H, V] of A3 / A4: integers in {-2..2} (bf16: {-1, 0, 1}, so that
    |dP - dsum| <= hd + 3 <= 131 needs 8 significant bits and 64 (dP - dsum) is exact in bf16) and dsum in {-3..3}."""
    N, H, V, hd = case
    r = 1 if bf16 else 2
    return int_values(case, 21, r, (N, V, H * hd)), int_values(case, 22, r), int_values(case, 23, 3, (N, H, V))


def b_scales(hd):
    """Check B runs at the network's 1 / sqrt(hd) (N(0, 1) operands: scores of standard deviation 1) and at 4 / sqrt(hd) (standard
    deviation 4: a few keys carry each row, the running maximum moves late and the rescale matters)."""
    return [("s1", hd ** -0.5), ("s4", 4.0 * hd ** -0.5)]


B_SEED = 6


def b_operands(case, bf16, seed=B_SEED):
    """q, k, v [N, H, V, hd] and dO [N, V, H hd] ~ N(0, 1), rounded to the storage type.
    The seed matters at V = 4 only: with scores of standard deviation 4 over 4 keys the softmax is nearly one-hot, dP - dsum nearly
    cancels and max |dQ|, |dK| can fall to 0.3 (typical: 3 to 9).  The bf16 rounding of the stored `out`, which feeds dsum = rowsum(dO out)
    before any backward kernel runs, then alone reaches 1.2 to 1.5 times the backward bound (seeds 5, 9, 12; with dsum from the unrounded
    out the same draws stay below 0.17 of it).  tests/test_attention_cpu.py holds the condition: the emulation is inside every bound."""
    N, H, V, hd = case
    q, k, v = (real_values(case, seed + i, bf16) for i in range(3))
    dout = real_values(case, seed + 3, bf16, (N, V, H * hd))
    return q, k, v, dout
