"""The checker of the down-gridding tests (tests/test_downgrid_cpu.py, tests/test_downgrid_gpu.py): a float64 numpy evaluation of
trilinear interpolation with align_corners=False semantics and the EXACT ratio S/T, written from the formula alone:

    per axis and output index d: coordinate max((d + 1/2) S/T - 1/2, 0) = max((2d + 1) S - T, 0) / (2T),
    i0 = floor, i1 = min(i0 + 1, S - 1), lambda = frac;   out = sum over the 8 corners of the product of (1 - lambda | lambda).

Index and lambda are taken from the integer quotient and remainder, so nothing depends on how a float coordinate rounds."""
import numpy as np

U = 2.0 ** -24                                   # unit roundoff of fp32 (relative to the magnitude; half an ulp)


def taps(S, T):
    d = np.arange(T, dtype=np.int64)
    num = np.maximum((2 * d + 1) * S - T, 0)
    i0 = num // (2 * T)
    lam = (num % (2 * T)).astype(np.float64) / (2.0 * T)
    assert i0.max() <= S - 1
    return i0, np.minimum(i0 + 1, S - 1), lam


def check_downgrid(x, T):
    """x: [n, S, S, S] -> (ref, lo, hi, amax) as float64 [n, T, T, T]: the interpolated value and, for every output voxel, the smallest,
    the largest and the largest-magnitude of its 8 corners."""
    x = np.asarray(x, dtype=np.float64)
    S = x.shape[-1]
    i0, i1, lam = taps(S, T)
    ref, lo, hi = x, x, x
    for axis in (1, 2, 3):
        shape = [1, 1, 1, 1]
        shape[axis] = T
        l = lam.reshape(shape)
        ref = np.take(ref, i0, axis=axis) * (1.0 - l) + np.take(ref, i1, axis=axis) * l
        lo = np.minimum(np.take(lo, i0, axis=axis), np.take(lo, i1, axis=axis))
        hi = np.maximum(np.take(hi, i0, axis=axis), np.take(hi, i1, axis=axis))
    return ref, lo, hi, np.maximum(np.abs(lo), np.abs(hi))


def kernel_bound(amax):
    """|out - ref| allowed to the HIP kernel: lambda and 1 - lambda rounded once per axis plus seven blends, each <= 2^-24 of the corner
    magnitude, rounded up to 16."""
    return 16 * U * amax


def interpolate_bound(S, lo, hi, amax):
    """|F.interpolate - ref| in fp32: torch evaluates the coordinate scale * (d + 0.5) - 0.5 in fp32, uncertain by up to 2 S 2^-24 in
    lambda per axis (three axes, times the corner range), plus the rounding of the blend."""
    return 6 * S * U * (hi - lo) + 24 * U * amax


def lognormal_cubes(n, S, seed):
    """Densities of dynamic range e^{+-8}: 1e10 exp(2 N(0, 1)), seeded."""
    g = np.random.default_rng(seed)
    return (1e10 * np.exp(2.0 * g.standard_normal((n, S, S, S)))).astype(np.float32)
