"""Helpers of the exact-integer kernel checks (tests/test_input_grad_kernels_gpu.py, tests/test_groupnorm_kernels_gpu.py,
tests/test_wgrad_kernels_gpu.py, tests/test_conv_kernels_gpu.py, tests/test_attention_kernels_gpu.py; their CPU halves): operands
that are small integers held as floats make every product and every partial sum an integer below 2^24, so fp32 addition is exact in
any order and a kernel must give the bits of the same sum computed in int64 / float64 on the CPU."""
import torch

DEV = "cuda:0"


def ints(shape, seed, terms):
    """Uniform integers in {-2..2} as fp32.  `terms` = the longest sum of products the case forms: 4 * terms must stay below 2^24, or
    fp32 addition is no longer exact in every order and check A would need a tolerance."""
    assert 4 * terms < 2 ** 24, f"exact-integer check: 4 x {terms} terms reaches 2^24, fp32 sums are no longer exact"
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g, dtype=torch.int8).float()


def ints_biased(shape, seed, terms):
    """Uniform integers in {0..3} as fp32: every product is >= 0, so a sum of `terms` products grows to about 2.25 * terms (signed
    data stays near sqrt(terms)) and an accumulator, LDS fold or slab kept in less than fp32 can no longer hold it exactly.
    9 * terms must stay below 2^24."""
    assert 9 * terms < 2 ** 24, f"exact-integer check: 9 x {terms} terms reaches 2^24, fp32 sums are no longer exact"
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 4, shape, generator=g, dtype=torch.int8).float()


def assert_same_bits(got, ref, what):
    """torch.equal with a report of where: the mismatch pattern (which voxels, which tile face, which sample) names the fault."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = [(tuple(i.tolist()), got[tuple(i)].item(), ref[tuple(i)].item()) for i in bad[:8]]
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} values differ; first (index, got, ref): {first}")


def in_sentinel(numel, shape, pad=64, value=-7777.0, dtype=torch.float32):
    """A contiguous view of `shape` (fp32 unless `dtype` says otherwise) in the middle of a larger sentinel-filled buffer; returns
    (buffer, view, check).  The sentinel is `value` rounded to `dtype`."""
    value = torch.tensor(value, dtype=dtype).item()
    buf = torch.full((numel + 2 * pad,), value, dtype=dtype, device=DEV)
    view = buf[pad:pad + numel].view(shape)

    def untouched():
        return bool((buf[:pad] == value).all().item() and (buf[pad + numel:] == value).all().item())
    return buf, view, untouched
