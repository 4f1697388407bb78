"""Inputs, checker and bounds shared by test_normalization_cpu.py and test_normalization_gpu.py.

The checker is the arithmetic of the reference's notebook (scripts/calc_normalization.ipynb) on the same float32 input:
    v = np.log10(x.astype(np.float64) + alpha);  v.mean();  v.std()
over the valid elements (x finite, x + alpha > 0).

The two inputs are the two regimes of the real fields:
  "cdm":  10 ** N(10.02, 0.55) - mean about 10, std 0.55, mean^2 / var about 330: where a careless accumulation shows;
  "star": 97 % exact zeros, the rest 10 ** N(1.5, 0.8) - mean about 0.05, most elements give log10(1) = 0 exactly."""
import functools
import os

import numpy as np

REL = 1e-11                                  # the bound of the issue; its derivation: test_normalization_gpu.test_kernel_matches_checker
N_BIG = 2 ** 20 + 3


@functools.lru_cache(maxsize=None)
def _values(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "cdm":
        x = (10.0 ** rng.normal(10.02, 0.55, n)).astype(np.float32)
    elif kind == "star":
        x = np.zeros(n, np.float32)
        some = rng.random(n) >= 0.97
        x[some] = (10.0 ** rng.normal(1.5, 0.8, int(some.sum()))).astype(np.float32)
    else:
        raise ValueError(kind)
    x.setflags(write=False)                  # shared between tests: never modified
    return x


def values(kind, n, seed=0):
    """n float32 values of the regime `kind` (read-only, cached: computed once per session)."""
    return _values(kind, int(n), int(seed))


def checker(x, alpha):
    """{"n", "mean", "std", "min", "max", "n_bad", "vmax"}: the notebook's three numpy lines over the valid elements of x."""
    x = np.asarray(x, np.float32).reshape(-1)
    t = x.astype(np.float64) + alpha
    ok = np.isfinite(x) & (t > 0)
    v = np.log10(t[ok])
    return {"n": int(ok.sum()), "mean": float(v.mean()), "std": float(v.std()), "min": float(x[ok].min()), "max": float(x[ok].max()),
            "n_bad": int((~ok).sum()), "vmax": float(np.abs(v).max())}


def assert_moments_close(mean, std, ref, what=""):
    """|mean - ref| <= 1e-11 max(|ref|, 1) (relative; absolute for a mean below 1 in magnitude) and |std - ref| <= 1e-11 |ref| plus
    the checker's own rounding floor 4 eps max|v|: np.std of n equal values v is not 0 but up to about eps |v| (its mean is rounded),
    so a purely relative bound on a std of (nearly) zero would test numpy, not the code."""
    e_mean, e_std = abs(mean - ref["mean"]), abs(std - ref["std"])
    b_mean = REL * max(abs(ref["mean"]), 1.0)
    b_std = REL * abs(ref["std"]) + 4 * np.finfo(np.float64).eps * ref["vmax"]
    print(f"{what}: mean {mean!r} (err {e_mean:.2e}, bound {b_mean:.2e}), std {std!r} (err {e_std:.2e}, bound {b_std:.2e})")
    assert e_mean <= b_mean, (what, "mean", mean, ref["mean"], e_mean)
    assert e_std <= b_std, (what, "std", std, ref["std"], e_std)


def write_stack(root, field, cubes, dataset_name="CMD"):
    """np.save of the stack `cubes` (n, S, S, S) at field_path(...) of the Astrid LH z=0 set; returns the path."""
    from vdm4cdm_amd import data
    p = data.field_path(root, dataset_name, "Astrid", "LH", "z_0.0", field)
    os.makedirs(os.path.dirname(p), exist_ok=True)
    np.save(p, np.asarray(cubes, np.float32))
    return p


def write_params(root, n_sims):
    from vdm4cdm_amd import data
    p = data.params_path(root, "Astrid", "LH")
    os.makedirs(os.path.dirname(p), exist_ok=True)
    np.savetxt(p, np.random.default_rng(7).uniform(0.1, 1.0, (n_sims, 6)))
    return p


def small_root(root, n_sims=2, S=16, fields=("Mgas", "Mcdm")):
    """A stand-in CAMELS directory: `n_sims` cubes of S^3 "cdm" values per field (another seed each) and the parameter table."""
    root = str(root)
    for i, c in enumerate(fields):
        write_stack(root, c, values("cdm", n_sims * S ** 3, seed=100 + i).reshape(n_sims, S, S, S))
    write_params(root, n_sims)
    return root
