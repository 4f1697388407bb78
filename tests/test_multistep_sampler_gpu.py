"""The deterministic multistep samplers on the HIP backend (sampling.hip_multistep_sampler: NetStep + K9m in the captured step): graph
against eager, against the float64-coefficient reference loop of tests/_multistep_ref.py driven by the oracle network, classifier-free
guidance, rows as chains of their own, the untouched defaults, flow matching at order 2 and the generate entry.  16^3, the smallest
network of the sampler tests.  Nothing here is a statement about sample quality: the weights are random."""
import pytest
import torch

import _multistep_cases as C
import _multistep_ref as R
from helpers import grf, oracle_cfg, oracle_params, randomize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_net(D=16, chs=(16, 32, 64), sc=1, vd=(6,), pm="zeros", precision="fp32", seed=1, zero_out=False):
    from vdm4cdm_amd.networks import CUNet
    net = CUNet(shape=(1, D, D, D), chs=list(chs), s_conditioning_channels=sc, v_conditioning_dims=list(vd), t_conditioning=True,
                norm_groups=8, mid_attn=False, dropout_prob=0.0, conv_padding_mode=pm, n_attention_heads=4, backend="hip",
                precision=precision)
    randomize(net, seed)
    if zero_out:                                             # eps_hat = 0 exactly at any batch size (tests/test_batched_sampling_gpu.py)
        with torch.no_grad():
            net.view("conv_out.weight").zero_()
            net.view("conv_out.bias").zero_()
    return net


def make_vdm(net, w_cfg=None):
    from vdm4cdm_amd.vdm_model import LightVDM
    return LightVDM(score_model=net, draw_figure=None, gamma_max=13.3, learning_rate=3e-4, w_cfg=w_cfg).to(DEV).eval()


def inputs(B, seed=3, D=16):
    g = torch.Generator().manual_seed(seed + 2)
    return grf((B, 1, D, D, D), seed), grf((B, 1, D, D, D), seed + 1), [torch.rand(B, 6, generator=g)]


def _kw(s, v):
    return dict(s_conditioning=s.to(DEV), v_conditionings=[a.to(DEV) for a in v])


# ------------------------------------------------------------------------------ 11. graph == eager
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_equals_eager(precision):
    vdm = make_vdm(make_net(precision=precision, **C.NET_CFG))
    _, s, v = inputs(2)
    z1 = grf((2, 1, 16, 16, 16), 60, slope=0.0)
    n = C.GRAPH_STEPS
    run = lambda **kw: vdm.draw_samples(batch_size=2, n_sampling_steps=n, z=z1.clone(), sampler="dpm2m", **_kw(s, v), **kw).cpu()
    graph, eager = run(use_graph=True), run(use_graph=False)
    assert graph.shape == (2, 1, 16, 16, 16) and torch.isfinite(graph).all() and torch.equal(graph, eager)
    stack = run(use_graph=True, return_all=True)
    assert stack.shape == (n, 2, 1, 16, 16, 16) and torch.equal(stack[-1], graph)
    assert torch.equal(run(use_graph=False, return_all=True), stack)
    assert not torch.equal(stack[0], stack[1])


# ------------------------------------------------------------------------------ 12. the reference loop with the oracle network
def test_sampler_matches_the_reference_loop():
    """fp32, n = 20, supplied z_1: |HIP - reference| <= 2e-5 max|ref| + 1e-3 for dpm2m and ddim (the tolerance of
    test_sampler_matches_oracle); the two samplers differ from each other by more than 10 times that, so the history term is tested."""
    from oracle import unet_oracle
    net = make_net(precision="fp32", **C.NET_CFG)
    vdm = make_vdm(net)
    n = C.ORACLE_STEPS
    _, s, v = inputs(1)
    z1 = grf((1, 1, 16, 16, 16), 60, slope=0.0)
    P = oracle_params(net)
    score = lambda z, tn: unet_oracle.cunet_forward(P, oracle_cfg(net), z, tn, s, v)
    out, ref = {}, {}
    for name, order in (("dpm2m", 2), ("ddim", 1)):
        out[name] = vdm.draw_samples(batch_size=1, n_sampling_steps=n, z=z1.clone(), sampler=name, **_kw(s, v)).cpu()
        with torch.no_grad():
            ref[name] = R.vdm_sample(score, z1.clone(), n, order=order)
        err, top = (out[name] - ref[name]).abs().max().item(), ref[name].abs().max().item()
        print(f"{name}: err {err:.3e}, max|ref| {top:.3e}, tolerance {C.sampler_tolerance(top):.3e}")
        assert torch.isfinite(ref[name]).all() and err <= C.sampler_tolerance(top), f"{name}: err {err} (max|ref| {top})"
    gap = (ref["dpm2m"] - ref["ddim"]).abs().max().item()
    assert gap > 10 * C.sampler_tolerance(ref["dpm2m"].abs().max().item()), f"dpm2m and ddim only differ by {gap}"
    assert (out["dpm2m"] - out["ddim"]).abs().max().item() > 10 * C.sampler_tolerance(ref["dpm2m"].abs().max().item())


# ------------------------------------------------------------------------------ 13. classifier-free guidance
def test_cfg_matches_the_reference_loop():
    from oracle import unet_oracle, vdm_oracle
    net = make_net(precision="fp32", **C.NET_CFG)
    vdm = make_vdm(net)
    n, w = C.CFG_STEPS, C.W_CFG
    _, s, v = inputs(1)
    z1 = grf((1, 1, 16, 16, 16), 61, slope=0.0)
    run = lambda: vdm.draw_samples(batch_size=1, n_sampling_steps=n, z=z1.clone(), sampler="dpm2m", **_kw(s, v)).cpu()
    plain = run()
    vdm.model.w_cfg = 0.0
    out0 = run()
    assert (out0 - plain).abs().max().item() <= 1e-5 * plain.abs().max().item(), "w_cfg = 0 differs from the unguided chain"
    vdm.model.w_cfg = w
    out = run()
    P = oracle_params(net)
    score_v = lambda z, tn, vv: unet_oracle.cunet_forward(P, oracle_cfg(net), z, tn, s, vv)
    with torch.no_grad():
        ref = R.vdm_sample(vdm_oracle.cfg_score_fn(score_v, v, w), z1.clone(), n, order=2)
    err, top = (out - ref).abs().max().item(), ref.abs().max().item()
    print(f"cfg: err {err:.3e}, max|ref| {top:.3e}")
    assert (ref - plain).abs().max().item() > 1e-2 * top, "guidance had no effect: the test would be vacuous"
    assert err <= C.sampler_tolerance(top), f"CFG sampler err {err} (max|ref| {top})"


# ------------------------------------------------------------------------------ 14. rows are chains
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "hipgraph"])
def test_rows_are_chains_of_their_own(use_graph):
    """seeds=[a, b, c]: row r is the batch-1 chain with seed=seeds[r], bit for bit, under the conditions
    test_batched_chains_equal_single_chains_on_a_zero_output_net asserts it for the ancestral sampler (chs (16, 32), conv_out zero, fp32;
    per-row conditioning)."""
    vdm = make_vdm(make_net(chs=(16, 32), zero_out=True))
    g = torch.Generator().manual_seed(4)
    s, v = torch.randn(3, 1, 16, 16, 16, generator=g).to(DEV), [torch.rand(3, 6, generator=g).to(DEV)]
    n = 4
    out = vdm.draw_samples(batch_size=3, n_sampling_steps=n, seeds=C.ROW_SEEDS, sampler="dpm2m", s_conditioning=s, v_conditionings=v,
                           use_graph=use_graph).cpu()
    assert out.shape == (3, 1, 16, 16, 16) and torch.isfinite(out).all() and not torch.equal(out[0], out[1])
    for r, sd in enumerate(C.ROW_SEEDS):
        one = vdm.draw_samples(batch_size=1, n_sampling_steps=n, seed=sd, sampler="dpm2m", s_conditioning=s[r:r + 1],
                               v_conditionings=[v[0][r:r + 1]], use_graph=use_graph).cpu()
        assert torch.equal(out[r:r + 1], one), f"chain {r} differs from the chain sampled alone"


# ------------------------------------------------------------------------------ 15. the defaults are untouched
def test_defaults_are_the_paths_of_before():
    from vdm4cdm_amd.sfm_model import LightSFM
    net = make_net(precision="fp32", **C.NET_CFG)
    vdm = make_vdm(net)
    _, s, v = inputs(1)
    kw = dict(batch_size=1, n_sampling_steps=5, seed=123, **_kw(s, v))
    a, b = vdm.draw_samples(**kw), vdm.draw_samples(sampler="ancestral", **kw)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, vdm.draw_samples(sampler="ddim", **kw))
    sfm = LightSFM(velocity_model=net, learning_rate=3e-4).to(DEV).eval()
    x0 = s.to(DEV)
    kw = dict(x0=x0, n_sampling_steps=6, v_conditionings=[a.to(DEV) for a in v])
    assert torch.equal(sfm.draw_samples(**kw), sfm.draw_samples(order=1, **kw))
    assert torch.equal(sfm.model.sample(x0, 6, v_conditionings=kw["v_conditionings"]),
                       sfm.model.sample(x0, 6, v_conditionings=kw["v_conditionings"], order=1))


# ------------------------------------------------------------------------------ 16. flow matching, order 2
def test_sfm_order_two():
    """The captured Adams-Bashforth 2 loop against the reference AB2 loop (tests/_multistep_ref.py) that evaluates the HIP network
    eagerly, at the tolerance test_sfm_loss_gradients_and_sampler_match_oracle uses for the Euler sampler (2e-4 max|ref| + 1e-4); the
    graph equals the eager launches bit for bit; AB2 differs from Euler."""
    from vdm4cdm_amd.sfm_model import LightSFM
    net = make_net(precision="fp32", **C.NET_CFG)
    sfm = LightSFM(velocity_model=net, learning_rate=3e-4).to(DEV).eval()
    n = 8
    _, x0, v = inputs(1)
    x0d, vd = x0.to(DEV), [a.to(DEV) for a in v]
    graph = sfm.draw_samples(x0=x0d, n_sampling_steps=n, v_conditionings=vd, order=2, use_graph=True)
    eager = sfm.draw_samples(x0=x0d, n_sampling_steps=n, v_conditionings=vd, order=2, use_graph=False)
    assert torch.isfinite(graph).all() and torch.equal(graph, eager)
    with torch.no_grad():
        vel = lambda i, x, r: sfm.model.velocity(x, torch.full((1,), r["t_norm"], device=DEV), x0d, vd)
        ref = R.run(R.sfm_rows(n, 2), x0d.clone(), vel)
        euler = R.run(R.sfm_rows(n, 1), x0d.clone(), vel)
    err, top = (graph - ref).abs().max().item(), ref.abs().max().item()
    print(f"sfm order 2: err {err:.3e}, max|ref| {top:.3e}, |ab2 - euler| {(ref - euler).abs().max().item():.3e}")
    assert err <= 2e-4 * top + 1e-4
    assert (ref - euler).abs().max().item() > 10 * (2e-4 * top + 1e-4), "AB2 and Euler coincide: the history term is untested"
    stack = sfm.draw_samples(x0=x0d, n_sampling_steps=n, v_conditionings=vd, order=2, return_all=True)
    assert stack.shape == (n, 1, 1, 16, 16, 16) and torch.equal(stack[-1], graph)


# ------------------------------------------------------------------------------ 17. the generate entry
def test_sample_repetitions_follow_the_sampler_variable(monkeypatch):
    """VDM4CDM_SAMPLER=dpm2m, 4 steps, 16^3: _sample_repetitions returns the cubes of draw_samples(sampler="dpm2m",
    seed=chain_seed(i)) - one chain per call on a random network; several per call on a zero-output network, where a row equals its
    chain sampled alone bit for bit."""
    from vdm4cdm_amd import entry
    monkeypatch.setenv("VDM4CDM_SAMPLER", "dpm2m")
    name = entry._sampler_name()
    assert name == "dpm2m"
    _, s, v = inputs(1)
    batch = {"conditioning": s, "conditioning_values": v}
    n, rep, first = C.ENTRY_STEPS, C.ENTRY_REP, 5
    for zero_out, per_call in ((False, 1), (True, 2)):
        vdm = make_vdm(make_net(chs=(16, 32), zero_out=zero_out))
        parts = entry._sample_repetitions(vdm, {"conditioning_values": 6}, batch, DEV, rep, first, 0, 1, n, per_call, name)
        assert [i for i, _ in parts] == list(range(rep))
        for i, cube in parts:
            want = vdm.draw_samples(batch_size=1, n_sampling_steps=n, seed=entry.chain_seed(first + i), sampler="dpm2m", **_kw(s, v))
            assert cube.shape == (1, 1, 16, 16, 16) and (cube == want.cpu().numpy()).all(), f"repetition {i}"
        default = entry._sample_repetitions(vdm, {"conditioning_values": 6}, batch, DEV, 1, first, 0, 1, n, 1)
        assert not (default[0][1] == parts[0][1]).all()      # the default is still the ancestral chain
    monkeypatch.delenv("VDM4CDM_SAMPLER")
    assert entry._sampler_name() == "ancestral"
