"""DDNM on the seed- / noise-keyed path, without a GPU: the host schedule against the eager loop, the coefficient tables against the
oracle's scalars, get_ddnm_result(noises=) on the torch backend against the reference fixture, the built-in operators, the argument
checks and the unchanged behaviour without the new keywords."""
import itertools
import types

import numpy as np
import pytest
import torch

from helpers import DD, DDNM_GOLD, replay_ddnm_case
from _ddnm_cases import fixture_noises, fixture_operator, fixture_vdm, residual

SCHEDULES = [(6, 0), (8, 2), (7, [0, 1, 2, 3, 2, 1, 0]), (250, 10)]


# ------------------------------------------------------------------------------ 1. host schedule
class _LoggingStream(DD.NoiseStream):
    """NoiseStream that also writes every draw into the event log."""

    def __init__(self, log):
        super().__init__(0)
        self.log = log

    def _draw(self, shape, device=None):
        self.log.append(("draw", self.calls))            # 0 is z_1; draw d of the schedule is call d + 1
        return super()._draw(shape, device)


class _LoggingModel:
    """`vdm.model` as the eager loop drives it: logs the grid indices of every (t, s) call."""

    def __init__(self, n, log):
        self.n, self.log = n, log
        self.score_model = types.SimpleNamespace(shape=(1, 2, 2, 2))

    def _k(self, t):
        return int(round((1.0 - float(t)) * self.n))

    def sample_zt_given_zs(self, zs, t, s):
        self.log.append(("travel", self._k(t), self._k(s)))
        return zs + 0.0 * torch.randn_like(zs)

    def sample_zs_given_zt(self, zt, t, s, return_ddnm=False, conditioning=None, **kwargs):
        assert return_ddnm and conditioning is None
        self.log.append(("eval", self._k(t), self._k(s)))
        return 1.0, 0.0, zt, 0.0


@pytest.mark.parametrize("n,l", SCHEDULES, ids=[f"n{n}" for n, _ in SCHEDULES])
def test_schedule_equals_the_eager_loops_calls_and_draws(n, l):
    """ddnm_schedule's (k, draw number) sequence is the sequence of (t, s) calls and noise draws of the existing eager loop."""
    from vdm4cdm_amd import utils
    from vdm4cdm_amd.vdm_model import ddnm_schedule
    log = []
    vdm = types.SimpleNamespace(device=torch.device("cpu"), model=_LoggingModel(n, log))
    y = torch.zeros(1, 1, 2, 2, 2)
    larr = l if isinstance(l, int) else np.asarray(l)
    with _LoggingStream(log) as ns:
        utils.get_ddnm_result(vdm, y, lambda x: x, lambda x: x, n_sampling_steps=n, l=larr)
    sch = ddnm_schedule(n, larr)
    want = [("draw", 0)]
    e = 0
    for i in range(n):
        L = sch["L"][i]
        want += [("travel", i - L, i), ("draw", sch["travel_draw"][i] + 1)]
        for _ in range(L + 1):
            assert sch["outer"][e] == i
            want += [("eval", sch["k"][e], sch["k"][e] + 1), ("draw", sch["draw"][e] + 1)]
            e += 1
    assert log == want
    ll = np.full(n, l) if isinstance(l, int) else np.asarray(l)
    assert e == len(sch["k"]) == sum(min(int(ll[i]), i) + 1 for i in range(n))
    assert ns.calls == 1 + sch["n_draws"]
    if (n, l) == (250, 10):
        assert len(sch["k"]) == 2695


def test_schedule_draw_count_equals_the_fixtures_noise_calls():
    from vdm4cdm_amd.vdm_model import ddnm_schedule
    for name, D, chs, seed, B, n, l, op, cond in DD.CASES:
        assert 1 + ddnm_schedule(n, l)["n_draws"] == int(DDNM_GOLD[f"{name}/noise_calls"][0]), name


# ------------------------------------------------------------------------------ 2. coefficient tables
@pytest.mark.parametrize("kind", ["fixed_linear", "learned_linear"])
def test_ddnm_tables_match_the_oracles_scalars(kind):
    """VDM.ddnm_tables against oracle/vdm_oracle.py's scalars of sample_zs_given_zt(return_ddnm=True) and sample_zt_given_zs.  Both
    sides are fp64 on the same fp32 grid and spell the same expressions: the observed difference is 0 on every entry (printed below).
    Bound: 2e-15 relative (9 ulps of fp64) - room for one differently rounded libm call (expm1, exp) per entry on another host, times
    ten."""
    from oracle import vdm_oracle
    from vdm4cdm_amd.vdm_model import VDM, ddnm_schedule
    vdm = VDM(torch.nn.Identity(), noise_schedule=kind)
    sched = vdm_oracle.Schedule(-13.3, 13.3)
    if kind == "learned_linear":
        with torch.no_grad():
            vdm.gamma_b.fill_(-11.0)
            vdm.gamma_w.fill_(-22.5)                     # |w| is what counts
        sched = vdm_oracle.Schedule(-13.3, 13.3, kind, b=-11.0, w=-22.5)
    n, l = 12, [0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 0]
    L = ddnm_schedule(n, l)["L"]
    coef, travel = vdm.ddnm_tables(n, L)
    assert coef.dtype == travel.dtype == torch.float64 and coef.shape == (n, 8) and travel.shape == (n, 2)
    steps = torch.linspace(1.0, 0.0, n + 1).double()
    worst = 0.0
    for k in range(n):
        c = vdm_oracle.step_coeffs(sched, steps[k], steps[k + 1])
        ref = torch.stack([1.0 / c["alpha_t"], c["sigma_t"], c["ratio"] * (1.0 - c["c"]), c["alpha_s"] * c["c"], c["scale"], c["t_norm"]])
        worst = max(worst, ((coef[k, :6] - ref).abs() / ref.abs().clamp(min=1e-300)).max().item())
        assert torch.all(coef[k, 6:] == 0)
        one = torch.ones(1, dtype=torch.float64)
        a = vdm_oracle.sample_zt_given_zs(sched, one, steps[k - L[k]], steps[k], 0.0 * one)      # a * 1 + b * 0
        b = vdm_oracle.sample_zt_given_zs(sched, 0.0 * one, steps[k - L[k]], steps[k], one)      # a * 0 + b * 1
        ref2 = torch.cat([a, b])
        worst = max(worst, ((travel[k] - ref2).abs() / ref2.abs().clamp(min=1.0)).max().item())
    print(f"ddnm_tables vs oracle ({kind}): worst relative difference {worst:.3e}")
    assert worst <= 2e-15
    assert travel[0, 0] == 1.0 and travel[0, 1] == 0.0      # L = 0: the travel is the identity, exactly


# ------------------------------------------------------------------------------ 3. noises= on the torch backend vs the fixture
@pytest.mark.parametrize("case", DD.CASES, ids=[c[0] for c in DD.CASES])
def test_noises_keyword_on_the_torch_backend_matches_the_fixture(case):
    """get_ddnm_result(noises=) - the fixture's stream as a list - gives the reference loop's result at the bound of
    test_ddnm_product_loop_matches_reference_golden (1e-4 max|gold|, residual 1e-3); with operator= instead of the callables too."""
    from vdm4cdm_amd import utils
    name, D, chs, seed, B, n, l, op, cond = case
    vdm, y, kw = fixture_vdm(case, "cpu", "torch")
    A, AT = DD.operators(op, (B, 1, D, D, D))
    gold = torch.from_numpy(DDNM_GOLD[f"{name}/x"])
    noises = fixture_noises(case)
    for variant in ("callables", "operator"):
        args = dict(A=A, AT=AT) if variant == "callables" else dict(operator=fixture_operator(case, "cpu"))
        x = utils.get_ddnm_result(vdm, y, n_sampling_steps=n, l=l, noises=noises, **args, **kw)
        err = (x - gold).abs().max().item()
        print(f"{name} [{variant}]: err {err:.3e} (bound {1e-4 * gold.abs().max().item():.3e}), residual {residual(A, x, y):.3e}")
        assert x.shape == gold.shape and err <= 1e-4 * gold.abs().max().item()
        assert residual(A, x, y) <= 1e-3
    x_all = utils.get_ddnm_result(vdm, y, A, AT, n_sampling_steps=n, l=l, noises=noises, return_all=True, **kw)
    assert x_all.shape == (n,) + tuple(gold.shape) and torch.equal(x_all[-1], x)
    np.testing.assert_allclose(x_all.abs().amax(dim=tuple(range(1, x_all.dim()))).numpy(), DDNM_GOLD[f"{name}/x_all_absmax"], rtol=1e-3)


def test_seeded_chains_on_the_torch_backend_do_not_depend_on_the_batch():
    from vdm4cdm_amd import utils
    case = DD.CASES[0]
    vdm, y, kw = fixture_vdm(case, "cpu", "torch")
    op = fixture_operator(case, "cpu")
    both = utils.get_ddnm_result(vdm, y, n_sampling_steps=4, l=1, seeds=[11, 12], operator=op)
    again = utils.get_ddnm_result(vdm, y, n_sampling_steps=4, l=1, seeds=[11, 12], operator=op)
    assert torch.equal(both, again)
    one = utils.get_ddnm_result(vdm, y[1:], n_sampling_steps=4, l=1, seeds=[12], operator=utils.MaskOperator(op.mask[1:]))
    assert (both[1:] - one).abs().max().item() <= 1e-4 * one.abs().max().item()       # (batch-size dependent conv rounding only)


# ------------------------------------------------------------------------------ 4. operators
def test_builtin_operators_reproduce_the_fixtures_callables():
    from vdm4cdm_amd import utils
    shape = (2, 1, 16, 16, 16)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    A, AT = DD.operators("pool", shape)
    op = utils.BlockMeanOperator((1, 1, 2))
    assert torch.equal(op.A(x), A(x)) and torch.equal(op.AT(A(x)), AT(A(x)))
    A, AT = DD.operators("mask", shape)
    m = torch.zeros(shape)
    m[..., :8] = 1.0
    op = utils.MaskOperator(m)
    assert torch.equal(op.A(x), A(x)) and torch.equal(op.AT(x), AT(x))


def test_block_mean_up_sampling_is_a_right_inverse():
    from vdm4cdm_amd import utils
    g = torch.Generator().manual_seed(5)
    for f in itertools.product((1, 2, 4, 8), repeat=3):
        op = utils.BlockMeanOperator(f)
        y = torch.randn((2, 1, 16 // f[0], 16 // f[1], 16 // f[2]), generator=g)
        up = op.AT(y)
        assert up.shape == (2, 1, 16, 16, 16)
        assert torch.equal(op.A(up), y), f
        x = torch.randn((1, 1, 16, 16, 16), generator=g).double()
        ref = x.reshape(1, 1, 16 // f[0], f[0], 16 // f[1], f[1], 16 // f[2], f[2]).mean(dim=(3, 5, 7))
        assert torch.allclose(op.A(x), ref, rtol=1e-13, atol=1e-15)


# ------------------------------------------------------------------------------ 5. argument errors, before any work
def test_argument_errors():
    from vdm4cdm_amd import utils
    case = DD.CASES[0]
    name, D, chs, seed, B, n, l, op, cond = case
    vdm, y, kw = fixture_vdm(case, "cpu", "torch")
    A, AT = DD.operators(op, (B, 1, D, D, D))
    noises = fixture_noises(case)
    with pytest.raises(ValueError, match="seeds"):
        utils.get_ddnm_result(vdm, y, A, AT, n_sampling_steps=n, l=l, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="noises"):
        utils.get_ddnm_result(vdm, y, A, AT, n_sampling_steps=n, l=l, noises=noises[:-1])
    with pytest.raises(ValueError, match="combined"):
        utils.get_ddnm_result(vdm, y, A, AT, n_sampling_steps=n, l=l, noises=noises, seed=1)
    with pytest.raises(ValueError, match="combined"):
        utils.get_ddnm_result(vdm, y, A, AT, n_sampling_steps=n, l=l, seeds=[1, 2], seed=1)
    vdm12 = types.SimpleNamespace(device=torch.device("cpu"), model=types.SimpleNamespace(score_model=types.SimpleNamespace(shape=(1, 12, 12, 12))))
    with pytest.raises(ValueError, match="divide"):          # 12 % 8 != 0; raised before the model is touched
        utils.get_ddnm_result(vdm12, torch.zeros(1, 1, 12, 12, 3), n_sampling_steps=4, l=0, seed=1, operator=utils.BlockMeanOperator((1, 1, 8)))
    with pytest.raises(ValueError, match="factors"):
        utils.BlockMeanOperator((1, 3, 2))
    with pytest.raises(ValueError, match="broadcast"):
        utils.get_ddnm_result(vdm, y, n_sampling_steps=n, l=l, seed=1, operator=utils.MaskOperator(torch.ones(1, 1, D, D, D + 1)))
    with pytest.raises(ValueError, match="A and AT"):
        utils.get_ddnm_result(vdm, y, n_sampling_steps=n, l=l, seed=1)
    with pytest.raises(ValueError, match="l must be"):
        utils.get_ddnm_result(vdm, y, A, AT, n_sampling_steps=n, l=[1, 2], seed=1)


# ------------------------------------------------------------------------------ 6. unchanged without the new keywords
@pytest.mark.parametrize("case", DD.CASES, ids=[c[0] for c in DD.CASES])
def test_without_new_keywords_the_eager_loop_is_unchanged(case):
    """The signature changed (A / AT optional, keyword-only additions); with none of them given the loop still draws noise_calls
    times from torch.randn / randn_like and returns the fixture's result (the property of
    test_ddnm_product_loop_matches_reference_golden; replay_ddnm_case asserts the draw count)."""
    x, gold, resid = replay_ddnm_case(case, "cpu", "torch")
    assert (x - gold).abs().max().item() <= 1e-4 * gold.abs().max().item() and resid <= 1e-3


# ------------------------------------------------------------------------------ 7. C-ABI argument checks (host side, no launch)
def test_cabi_argument_errors_of_the_ddnm_entries(hip_lib):
    import ctypes as C
    from vdm4cdm_amd._lib import DdnmTables
    p = 4096                                             # a non-null, 16-byte aligned address: every call returns before it launches
    t = DdnmTables(coef=p, sched=p, cursor=p, n_coef=4, n_sched=4, seeds=p, batch_stream=0, reserved=0)
    ref = C.byref(t)
    err = lambda: hip_lib.vdm_last_error()
    assert hip_lib.vdm_ddnm_blockmean_step(p, p, None, 0.0, p, 1, 8, 8, 8, 3, 1, 1, None, ref, None, 1, None) == -1 and b"factor" in err()
    assert hip_lib.vdm_ddnm_blockmean_step(p, p, None, 0.0, p, 1, 12, 8, 8, 8, 1, 1, None, ref, None, 1, None) == -1 and b"divide" in err()
    assert hip_lib.vdm_ddnm_blockmean_step(p, p, None, 0.0, p, 1, 8, 8, 6, 1, 1, 2, None, ref, None, 1, None) == -1 and b"multiple of 4" in err()
    assert hip_lib.vdm_ddnm_blockmean_step(p, p, None, 0.0, p, 2, 8, 8, 8, 1, 1, 2, None, ref, None, 3, None) == -1 and b"y_rows" in err()
    assert hip_lib.vdm_ddnm_mask_step(p, p, None, 0.0, p, 2, p, 1, None, ref, None, 3, 64, None) == -1 and b"mask_rows" in err()
    assert hip_lib.vdm_ddnm_mask_step(p, p, None, 0.0, p, 1, p, 1, None, ref, None, 1, 66, None) == -1 and b"per_row" in err()
    assert hip_lib.vdm_ddnm_mask_step(p + 4, p, None, 0.0, p, 1, p, 1, None, ref, None, 1, 64, None) == -1 and b"aligned" in err()
    assert hip_lib.vdm_ddnm_update(p, p, p, p, 2, None, ref, None, 3, 64, None) == -1 and b"aty_rows" in err()
    assert hip_lib.vdm_ddnm_update(p, p, None, p, 1, None, ref, None, 1, 64, None) == -1 and b"null" in err()
    assert hip_lib.vdm_ddnm_x0(p, p, None, 0.0, ref, p, 6, None) == -1 and b"multiple of 4" in err()
    assert hip_lib.vdm_ddnm_x0(p, p, None, 0.0, None, p, 8, None) == -1 and b"tables" in err()
    no_seeds = DdnmTables(coef=p, sched=p, cursor=p, n_coef=4, n_sched=4, seeds=None, batch_stream=0, reserved=0)
    assert hip_lib.vdm_ddnm_update(p, p, p, p, 1, None, C.byref(no_seeds), None, 1, 64, None) == -1 and b"seed table" in err()
    assert hip_lib.vdm_ddnm_travel(p, None, C.byref(no_seeds), p, 0, 0, 1, 64, None) == -1 and b"seed table" in err()
    assert hip_lib.vdm_ddnm_travel(p, None, ref, p, -1, 0, 1, 64, None) == -1
    assert hip_lib.vdm_ddnm_advance(None, p, 4, p, None) == -1 and hip_lib.vdm_ddnm_advance(p, p, 0, p, None) == -1
