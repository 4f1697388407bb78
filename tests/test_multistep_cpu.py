"""Deterministic multistep samplers on the CPU: the coefficient tables (VDM.multistep_table, SFM.multistep_table) against the float64
reference of tests/_multistep_ref.py, their order of convergence on problems with a closed-form answer, the interface refusals, the
argument errors of vdm_multistep_step (no launch) and the torch-backend loop.  The reference is the yardstick everywhere; it does not
import the product's table code.  None of this says anything about sample quality with trained weights."""
import os
import subprocess
import sys

import pytest
import torch
import yaml

import _multistep_cases as C
import _multistep_ref as R
from helpers import oracle_cfg, oracle_params, randomize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (1, 8, 8, 8)


def _net(vd=(6,)):
    from vdm4cdm_amd.networks import CUNet
    return CUNet(shape=SHAPE, chs=[8, 16], s_conditioning_channels=1, v_conditioning_dims=list(vd), norm_groups=4, backend="torch")


def _vdm(schedule):
    from vdm4cdm_amd.vdm_model import VDM
    m = VDM(_net(), noise_schedule=schedule)
    if schedule == "learned_linear":                         # (off the default endpoints, so that the learned parameters are what is read)
        with torch.no_grad():
            m.gamma_b.fill_(-11.0)
            m.gamma_w.fill_(-20.5)                            # gamma = b + |w| t
    return m


def _ref_rows(schedule, n, order, lof):
    """t_norm is (gamma - gamma_min) / (gamma_max - gamma_min) with the model's fixed endpoints under either schedule."""
    if schedule == "fixed_linear":
        return R.vdm_rows(n, order, lof)
    rows = R.vdm_rows(n, order, lof, gamma_min=-11.0, gamma_max=9.5)
    g = R.gamma_grid(n, -11.0, 9.5)
    for i, r in enumerate(rows):
        r["t_norm"] = (float(g[i]) + 13.3) / 26.6
    return rows


# ------------------------------------------------------------------------------ 1. the VDM table
@pytest.mark.parametrize("schedule", ["fixed_linear", "learned_linear"])
@pytest.mark.parametrize("n", C.TABLE_NS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("lof", [True, False], ids=["lower_order_final", "second_order_final"])
def test_vdm_multistep_table_matches_the_reference(schedule, n, order, lof):
    tab = _vdm(schedule).multistep_table(n, order=order, lower_order_final=lof)
    ref = R.as_table(_ref_rows(schedule, n, order, lof))
    assert tab.shape == (n, 8) and tab.dtype == torch.float64
    assert torch.allclose(tab, ref, rtol=C.TABLE_RTOL, atol=C.TABLE_ATOL), (tab - ref).abs().max().item()
    second = R.second_order_rows(n, order, lof)
    assert tab[0, 4].item() == 0.0                           # row 0 has no history: w_p == 0 exactly
    if lof:
        assert tab[n - 1, 4].item() == 0.0
    if order == 1 or n == 1 or (n == 2 and lof):
        assert not any(second) and (tab[:, 4] == 0.0).all()
    for i in range(n):
        assert (tab[i, 4].item() != 0.0) == second[i], i
    assert (tab[:, 6:] == 0.0).all()


def test_r_comes_from_the_grid():
    """The fp32 linspace is not exactly uniform in float64: r = h_prev / h differs from 1 in some row, and the table follows it."""
    rows = R.vdm_rows(10, 2, False)
    rs = [rows[i - 1]["h"] / rows[i]["h"] for i in range(1, 10)]
    assert any(r != 1.0 for r in rs)
    tab = _vdm("fixed_linear").multistep_table(10, order=2, lower_order_final=False)
    b = tab[1:, 3] + tab[1:, 4]                              # w_x + w_p = B
    assert torch.allclose(-tab[1:, 4] / b, 0.5 / torch.tensor(rs, dtype=torch.float64), rtol=1e-10, atol=0)


# ------------------------------------------------------------------------------ 2. a first-order row is the DDIM step
@pytest.mark.parametrize("schedule", ["fixed_linear", "learned_linear"])
def test_first_order_rows_are_the_ddim_step(schedule):
    """w_z + w_x e_z = alpha_s / alpha_t and w_x e_e = sigma_s - alpha_s sigma_t / alpha_t: the step is alpha_s x_hat + sigma_s eps_hat.
    alpha_s / alpha_t is column 0 of step_table; sigma_t = c sigma_t / c with c = -expm1(gamma_s - gamma_t) from the reference grid."""
    m = _vdm(schedule)
    n = 10
    tab, st = m.multistep_table(n, order=1), m.step_table(n)
    ref = _ref_rows(schedule, n, 1, True)
    a_s = torch.tensor([r["alpha_s"] for r in ref], dtype=torch.float64)
    s_s = torch.tensor([r["sigma_s"] for r in ref], dtype=torch.float64)
    e_z, e_e, w_z, w_x = tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3]
    ratio = st[:, 0]
    c = torch.tensor([-torch.expm1(torch.tensor(-2.0 * r["h"], dtype=torch.float64)).item() for r in ref], dtype=torch.float64)
    s_t = st[:, 1] / c
    assert torch.allclose(w_z + w_x * e_z, ratio, rtol=C.TABLE_RTOL, atol=C.TABLE_ATOL)
    assert torch.allclose(w_x * e_e, s_s - a_s * s_t * e_z, rtol=C.TABLE_RTOL, atol=C.TABLE_ATOL)
    assert torch.allclose(tab[:, 5], st[:, 3], rtol=C.TABLE_RTOL, atol=C.TABLE_ATOL)


# ------------------------------------------------------------------------------ 3. order of convergence (VDM)
@pytest.mark.parametrize("s", C.PRIOR_STDS)
def test_vdm_table_converges_at_its_order(s):
    """Scalar float64 chain over the PRODUCT's table with the analytic denoiser of a Gaussian prior, against the exact probability-flow
    solution.  The reference alone gives ratios 3.96, 3.99 (2M), 1.97, 1.99 (DDIM) and err_2M(64) = 2.66e-3 < err_DDIM(512) = 6.47e-3
    at s = 0.5."""
    m = _vdm("fixed_linear")
    err = {(o, n): R.gaussian_error(R.rows_of_table(m.multistep_table(n, order=o)), s) for o in (1, 2) for n in C.CONVERGENCE_NS}
    print({k: f"{v:.3e}" for k, v in err.items()})
    for a, b in ((64, 128), (128, 256)):
        lo, hi = C.SECOND_ORDER_RATIO
        assert lo <= err[2, a] / err[2, b] <= hi, (a, b, err[2, a] / err[2, b])
        lo, hi = C.FIRST_ORDER_RATIO
        assert lo <= err[1, a] / err[1, b] <= hi, (a, b, err[1, a] / err[1, b])
    assert err[2, 64] < err[1, 512]


def test_reference_convergence_figures():
    """The figures the product is held to are the reference's own (s = 0.5)."""
    e = {(o, n): R.gaussian_error(R.vdm_rows(n, o), 0.5) for o in (1, 2) for n in C.CONVERGENCE_NS}
    assert e[2, 64] == pytest.approx(2.66e-3, rel=5e-3) and e[1, 512] == pytest.approx(6.47e-3, rel=5e-3)
    assert e[2, 64] / e[2, 128] == pytest.approx(3.96, abs=0.01) and e[1, 64] / e[1, 128] == pytest.approx(1.97, abs=0.01)


# ------------------------------------------------------------------------------ 4. the SFM table
def test_sfm_multistep_table():
    from vdm4cdm_amd.sfm_model import SFM
    for n in C.TABLE_NS:
        for order in (1, 2):
            tab = SFM.multistep_table(n, order=order)
            assert tab.shape == (n, 8) and tab.dtype == torch.float64
            assert torch.allclose(tab, R.as_table(R.sfm_rows(n, order)), rtol=C.TABLE_RTOL, atol=C.TABLE_ATOL)
            assert tab[0, 4].item() == 0.0 and tab[0, 3].item() == 1.0 / n
    err = {(o, n): R.linear_ode_error(R.rows_of_table(SFM.multistep_table(n, order=o))) for o in (1, 2) for n in (64, 128, 256)}
    print({k: f"{v:.3e}" for k, v in err.items()})
    for a, b in ((64, 128), (128, 256)):
        assert C.SECOND_ORDER_RATIO[0] <= err[2, a] / err[2, b] <= C.SECOND_ORDER_RATIO[1], err[2, a] / err[2, b]
        assert C.FIRST_ORDER_RATIO[0] <= err[1, a] / err[1, b] <= C.FIRST_ORDER_RATIO[1], err[1, a] / err[1, b]
    # order 1 is SFM.step_table {1, -dt, 0, t_i}: x <- 1 * (x - (-dt) v), the same step and network time
    n = 10
    one, st = SFM.multistep_table(n, order=1), SFM.step_table(n)
    assert torch.equal(one[:, 3], -st[:, 1]) and torch.equal(one[:, 5], st[:, 3]) and torch.equal(one[:, 2], st[:, 0])
    assert (one[:, 4] == 0).all() and (one[:, 0] == 0).all() and (one[:, 1] == 1).all()


# ------------------------------------------------------------------------------ 5. refusals
def test_interface_refusals():
    from vdm4cdm_amd.sfm_model import LightSFM
    from vdm4cdm_amd.vdm_model import LightVDM
    vdm = LightVDM(score_model=randomize(_net(), 1), gamma_max=13.3).eval()
    s, v = torch.zeros(1, *SHAPE), [torch.zeros(1, 6)]
    kw = dict(batch_size=1, n_sampling_steps=3, s_conditioning=s, v_conditionings=v)
    with pytest.raises(ValueError, match="sampler"):
        vdm.draw_samples(sampler="heun", **kw)
    for name in ("ddim", "dpm2m"):
        with pytest.raises(ValueError, match="noises"):
            vdm.draw_samples(sampler=name, noises=[torch.zeros(1, *SHAPE)] * 3, **kw)
    with pytest.raises(ValueError, match="order"):
        vdm.model.multistep_table(4, order=3)
    sfm = LightSFM(velocity_model=randomize(_net(), 2)).eval()
    with pytest.raises(ValueError, match="order"):
        sfm.draw_samples(x0=s, n_sampling_steps=3, v_conditionings=v, order=3)
    with pytest.raises(ValueError, match="order"):
        sfm.model.multistep_table(4, order=3)


def _generate(tmp_path, out, sampler, steps="3"):
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "configs.yaml")))
    cfgs["VDM_Mstar_Mcdm_c_c_128"].update(cropsize=8, chs=[8, 16], ckpt_path=str(tmp_path / "none.ckpt"))
    p = tmp_path / "configs.yaml"
    yaml.safe_dump(cfgs, open(p, "w"))
    code = ("import sys; sys.path.insert(0, %r); from vdm4cdm_amd import entry; entry.generate_3d(['VDM_Mstar_Mcdm_c_c_128', %r, 'CV_1_128'], "
            "configs_path=%r)" % (ROOT, str(out), str(p)))
    env = dict({k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}, OMP_NUM_THREADS="2",
               VDM4CDM_BACKEND="torch", VDM4CDM_SAMPLING_STEPS=steps, VDM4CDM_REP="2", VDM4CDM_SAMPLER=sampler)
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)


def test_bad_sampler_variable_is_refused_before_any_model_is_built(tmp_path):
    r = _generate(tmp_path, tmp_path / "bad", "euler")
    assert r.returncode != 0 and "VDM4CDM_SAMPLER" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "bad").exists()                    # rejected before any output (and any model or GPU work)


def test_sampler_variable_selects_the_sampler_of_generate_3d(tmp_path):
    """dpm2m and ddim write different cubes from the same chain seeds (the same z_1), both finite; the variable reaches the sampler."""
    import numpy as np
    out = {}
    for name in ("dpm2m", "ddim"):
        r = _generate(tmp_path, tmp_path / name, name, steps="4")
        assert r.returncode == 0, r.stderr[-3000:]
        out[name] = np.load(tmp_path / name / "gen_0.npy")
        assert out[name].shape == (2, 1, 8, 8, 8) and np.isfinite(out[name]).all()
    assert not np.array_equal(out["dpm2m"], out["ddim"]) and not np.array_equal(out["dpm2m"][0], out["dpm2m"][1])


# ------------------------------------------------------------------------------ 6. the C entry point's argument errors
def test_multistep_step_argument_errors_do_not_need_a_gpu(hip_lib):
    import ctypes
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(z=p, eh=p, prev=p, coef=p, step=p)
    for missing in ok:
        a = dict(ok, **{missing: None})
        assert hip_lib.vdm_multistep_step(a["z"], a["eh"], None, 0.0, a["prev"], a["coef"], a["step"], 4, None) == -1, missing
        assert b"multistep_step" in hip_lib.vdm_last_error()
    for n in (0, -4):
        assert hip_lib.vdm_multistep_step(p, p, None, 0.0, p, p, p, n, None) == -1      # VDM_ERR_ARG, no launch
        assert b"multistep_step" in hip_lib.vdm_last_error()


# ------------------------------------------------------------------------------ 7. the torch backend
@pytest.mark.parametrize("name,order", [("dpm2m", 2), ("ddim", 1)])
def test_torch_backend_sampler_matches_the_reference_loop(name, order):
    """sample(sampler=) on the torch backend, 8^3, n = 20, against the reference loop (float64 scalars from the log-SNR formulas, the
    oracle network) from the same z_1: |d| <= 2e-5 max|ref| + 1e-3, the tolerance of test_sampler_matches_oracle."""
    from oracle import unet_oracle
    from vdm4cdm_amd.vdm_model import LightVDM
    net = randomize(_net(), 5)
    vdm = LightVDM(score_model=net, gamma_max=13.3).eval()
    g = torch.Generator().manual_seed(1)
    B, n = 2, 20
    z1, s, v = torch.randn(B, *SHAPE, generator=g), torch.randn(B, *SHAPE, generator=g), [torch.rand(B, 6, generator=g)]
    P = oracle_params(net)
    score = lambda z, tn: unet_oracle.cunet_forward(P, oracle_cfg(net), z, tn, s, v)
    with torch.no_grad():
        out = vdm.draw_samples(batch_size=B, n_sampling_steps=n, z=z1.clone(), sampler=name, s_conditioning=s, v_conditionings=v)
        ref = R.vdm_sample(score, z1.clone(), n, order=order)
        stack = vdm.draw_samples(batch_size=B, n_sampling_steps=n, z=z1.clone(), sampler=name, return_all=True, s_conditioning=s,
                                 v_conditionings=v)
    err, top = (out - ref).abs().max().item(), ref.abs().max().item()
    print(f"{name}: err {err:.3e}, max|ref| {top:.3e}")
    assert out.shape == (B, *SHAPE) and torch.isfinite(ref).all()
    assert err <= C.sampler_tolerance(top), f"err {err} (max|ref| {top})"
    assert stack.shape == (n, B, *SHAPE) and torch.equal(stack[-1], out)


def test_torch_backend_seeds_and_sfm_order_two():
    """seeds=: every row is the batch-1 chain of its seed (the deterministic samplers key z_1 as the ancestral one does); SFM order=2 on
    the torch backend against the reference AB2 loop with the oracle network; order=1 is the default path bit for bit."""
    from oracle import unet_oracle
    from vdm4cdm_amd.sfm_model import LightSFM
    from vdm4cdm_amd.vdm_model import LightVDM
    net = randomize(_net(), 5)
    vdm = LightVDM(score_model=net, gamma_max=13.3).eval()
    g = torch.Generator().manual_seed(2)
    s, v = torch.randn(1, *SHAPE, generator=g), [torch.rand(1, 6, generator=g)]
    with torch.no_grad():
        rows = vdm.draw_samples(batch_size=2, n_sampling_steps=4, seeds=[5, 9], sampler="dpm2m", s_conditioning=s.expand(2, -1, -1, -1, -1),
                                v_conditionings=[v[0].expand(2, -1)])
        one = vdm.draw_samples(batch_size=1, n_sampling_steps=4, seed=9, sampler="dpm2m", s_conditioning=s, v_conditionings=v)
        assert (rows[1:] - one).abs().max().item() <= 1e-5 * one.abs().max().item()
        net2 = randomize(_net(), 2)
        sfm = LightSFM(velocity_model=net2).eval()
        x0 = torch.randn(2, *SHAPE, generator=g)
        vv = [torch.rand(2, 6, generator=g)]
        P = oracle_params(net2)
        n = 6
        vel = lambda i, x, r: unet_oracle.cunet_forward(P, oracle_cfg(net2), x, torch.full((2,), r["t_norm"]), x0, vv)
        out = sfm.draw_samples(x0=x0, n_sampling_steps=n, v_conditionings=vv, order=2)
        ref = R.run(R.sfm_rows(n, 2), x0.clone(), vel)
        assert (out - ref).abs().max().item() < 1e-4         # the torch-backend Euler tolerance of test_cpu.py
        euler = R.run(R.sfm_rows(n, 1), x0.clone(), vel)
        assert (ref - euler).abs().max().item() > 1e-3       # ... and the history term is live
        assert torch.equal(sfm.draw_samples(x0=x0, n_sampling_steps=n, v_conditionings=vv, order=1),
                           sfm.draw_samples(x0=x0, n_sampling_steps=n, v_conditionings=vv))
        stack = sfm.draw_samples(x0=x0, n_sampling_steps=n, v_conditionings=vv, order=2, return_all=True)
        assert stack.shape == (n, 2, *SHAPE) and torch.equal(stack[-1], out)
