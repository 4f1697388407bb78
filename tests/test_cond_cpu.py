"""The host-only half of the K6 parity tests (device half: tests/test_cond_kernels_gpu.py; csrc/cond.hip): the cases sit on the code
edges they are named for, the float64 reference is the model's own operation, check A agrees with itself, an fp32 emulation of the
kernels' order of operations passes bound B, every emulated fault breaks check A, exceeds bound B or both, and the entry points refuse
what they must refuse before any launch.

Emulated faults (tests/_cond_ref.py emulate(fault=...)) over the ten cases: cases in which check A's bits break / cases in which bound
B is exceeded, and the range of the worst err / bound over the latter:
  last element of a dot product dropped         A 10  B 10   870 .. 3.6e6
  scalar tail dropped (len % 4 != 0)            A  6  B  6   2.2e6 .. 4.1e6      (the six cases with such a length; none elsewhere)
  forward slab boundary off by one              A  7  B  7   inf (an unwritten column)   (the cases with width >= 64)
  backward slab boundary off by one             A 10  B 10   1.7e3 .. 7.2e5
  second fold pass dropped                      A  3  B  3   3.6e3 .. 1.4e4      (the three cases that have one)
  dgelu taken at h1 where h2 belongs            A 10  B 10   1.2e3 .. 8.3e5
  the 1/2 at 0 missing                          A 10  B  0   -                   (random reals never hit 0: check A alone sees it)
  tanh approximation in place of erf            A  0  B 10   1.8 .. 398          (the tanh form saturates like erf: bound B alone)
  saved offset of mlp k with mlp 0's sizes      A  1  B  1   inf                 (the case with uneven sizes)
  dtable read with stride width                 A  9  B  9   inf (a NaN of the frame is read)   (every case with rows > 1)
  sin and cos halves exchanged                  A  4  B  4   1.5e6 ..            (the four cases with a sinusoid)
  i / (half - 1) in the frequency law           A  1  B  4   1.3e4 .. inf        (check A runs at t = 0: the embedding check of B)
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _cond_cases as W
import _cond_ref as R

_cache = {}


def operands(case):
    """(check A's operands, their int64 reference, check B's operands): computed once, shared, never changed"""
    if case.name not in _cache:
        a = W.ops_a(case, R.accept_a)
        _cache[case.name] = (a, R.ref_int(a)[0], W.ops_b(case))
    return _cache[case.name]


def check_b(ops, got):
    """worst err / bound over all tensors, the embedding's own check included"""
    worst = 0.0
    for k, m in enumerate(ops["mlps"]):
        if m["sinusoid"]:
            r = (got[f"{k}.emb"].double() - R.embed64(m["input"], m["in_dim"])).abs() / R.embed_bound(m["input"], m["in_dim"])
            worst = max(worst, float("inf") if bool(torch.isnan(r).any()) else r.max().item())
    ref = R.ref64(ops, [got[f"{k}.emb"] for k in range(len(ops["mlps"]))])
    rat = R.worst_by_tensor(R.ratios(got, ref, R.bounds(ops, ref)))
    return max(worst, max(rat.values())), rat


# ------------------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_case_sits_on_its_edge(case, hip_lib):
    """Every property a case is there for, recomputed from the restated constants; the restated buffer sizes equal the library's."""
    from vdm4cdm_amd._lib import CondMlp
    p = W.props(case)
    for key, want in case.expect.items():
        assert p[key] == want, f"{case.name}: {key} is {p[key]}, the case table says {want} ({case.edge})"
    assert 0 < len(case.mlps) <= W.COND_MAX and 0 < case.rows <= W.MAX_ROWS
    arr = (CondMlp * len(case.mlps))()
    for d, m in zip(arr, case.mlps):
        assert 0 < m.in_dim <= W.COND_MAXDIM and 0 < m.dim <= W.COND_MAXDIM and (not m.sinusoid or m.in_dim % 2 == 0)
        d.in_dim, d.dim, d.sinusoid = m.in_dim, m.dim, int(m.sinusoid)
    assert hip_lib.vdm_cond_saved_floats(arr, len(case.mlps), case.rows) == W.saved_floats(case)
    assert hip_lib.vdm_cond_bwd_scratch_floats(arr, len(case.mlps), case.rows, case.width) == W.scratch_floats(case)


def test_case_table_covers_the_paths():
    ps = [W.props(c) for c in W.CASES]
    assert {tp for p in ps for tp in p["tpo"]} == {1, 2, 4}
    assert any(p["param_trips"] == 2 for p in ps) and any(max(p["fold_passes"]) == 2 for p in ps)
    assert any(p["n"] == W.COND_MAX for p in ps) and any(p["last_fslab"] == 1 and p["fslabs"] > 1 for p in ps)
    assert any(p["last_bslab"] == 1 and p["bslabs"] > 1 for p in ps)
    # the lane chains the bound counts: quads cost four fmas each, the tail is shared
    assert W.chain(1, 4) == 1 and W.chain(3, 2) == 2 and W.chain(128, 2) == 64 and W.chain(132, 1) == 132 and W.chain(64, 4) == 16
    assert W.chain(8, 4) == 4 and W.chain(6, 4) == 2 and W.chain(65, 2) == 33
    assert (W.K_ERF, W.K_SINCOS, W.K_FREQ) == (4 * W.ERF_ERR_MEASURED, 4 * W.SINCOS_ERR_MEASURED, 4 * W.FREQ_ERR_MEASURED)


# ------------------------------------------------------------------------------------------------------------------- the reference
def test_reference_is_the_oracles_operation():
    """ref64 against oracle.unet_oracle's own functions with autograd, in float64, on a CUNet-shaped case (chs[0] = 32: t 64 -> 128 and
    a 6-vector -> 128, every block's projection stacked to one table)."""
    from oracle import unet_oracle as O
    case = W.Case("cunet", [W.t(64, 128), W.v(6, 128)], 4, 96, "", {})
    ops = W.ops_b(case)
    tv = ops["mlps"][0]["input"]
    emb32 = O.sinusoidal_embedding(tv, 64)
    assert bool(((emb32.double() - R.embed64(tv, 64)).abs() <= R.embed_bound(tv, 64)).all())
    t64 = tv.double().requires_grad_(True)
    arg = 1000.0 * t64[:, None] * R.freqs64(32)[None, :]
    xs = [torch.cat([torch.sin(arg), torch.cos(arg)], 1), ops["mlps"][1]["input"].double().requires_grad_(True)]
    ref = R.ref64(ops)
    params, table = [], 0.0
    for k, m in enumerate(ops["mlps"]):
        p = {f"m.{j}.{n}": m[key].double().requires_grad_(True) for j, n, key in ((0, "weight", "w1"), (0, "bias", "b1"), (2, "weight", "w2"),
                                                                                 (2, "bias", "b2"))}
        p["proj"] = m["wproj"].double().requires_grad_(True)
        params.append(p)
        table = table + F.linear(O._mlp2(p, "m", xs[k]), p["proj"])
    bias = torch.zeros(case.width, dtype=torch.float64, requires_grad=True)
    ((table + bias) * ops["dtable"].double()).sum().backward()

    def close(a, b, what):
        assert (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1.0), what

    close(ref["table"], table.detach(), "table")
    close(ref["dbias"], bias.grad, "dbias")
    close(ref["0.din"], t64.grad, "dL/dt")
    close(ref["1.din"], xs[1].grad, "dL/dv")
    for k, p in enumerate(params):
        for key, name in (("dw1", "m.0.weight"), ("db1", "m.0.bias"), ("dw2", "m.2.weight"), ("db2", "m.2.bias"), ("dwproj", "proj")):
            close(ref[f"{k}.{key}"], p[name].grad, f"{k}.{key}")


# ------------------------------------------------------------------------------------------------------------------- check A
@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_check_a_agrees_with_itself(case):
    """The four conditions hold (ref_int asserts them: exact sums, covered columns, all three signs of h1 and h2, a backward half
    that is nowhere identically 0 and uses the slope 1/2 in both layers); the float64 erf reference, rounded to fp32, has the bits of the int64 ReLU
    reference (float64 itself keeps exp(-128) = 2.6e-56 in gelu' where fp32 has an exact 0: the only difference); torch's fp32 erf
    gives ReLU bit for bit; the fp32 emulation of the kernels' order has the reference's bits."""
    ops, ref, _ = operands(case)
    _, info = R.ref_int(ops)
    assert info["big"] < R.EXACT_LIMIT and info["cover"] and all(min(s) > 0 for s in info["signs"].values())
    assert not info["dead"] and all(info["half_used"].values()) and info["layers_differ"]
    for key in ref:                                       # the fourth condition once more, from the reference itself
        assert key.split(".")[-1] not in R.BACKWARD or bool((ref[key] != 0).any()), f"{key} is all 0: check A would compare 0 with 0"
    r64 = R.ref64(ops)
    emu = R.emulate(ops)
    for key, want in ref.items():
        assert torch.equal(r64[key].float().double(), want), f"float64 erf reference: {key}"
        assert torch.equal(emu[key].double(), want), f"fp32 emulation: {key}"
    for k in range(len(case.mlps)):
        h = ref[f"{k}.h2"].float()
        assert torch.equal(R.gelu32(h), h.clamp(min=0)) and torch.equal(R.dgelu32(h), 0.5 * (1 + torch.sign(h)))


# ------------------------------------------------------------------------------------------------------------------- check B
@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_emulation_passes_bound_b(case):
    _, _, ops = operands(case)
    worst, rat = check_b(ops, R.emulate(ops))
    print(f"\n  {case.name:<13}" + " ".join(f"{key}={r:.3f}" for key, r in rat.items()))
    assert worst <= 1.0, rat


def test_bound_terms():
    """The pieces of the bound against brute force: gelu'' and gelu' stay inside their Lipschitz constants, the evaluation-error models
    are positive and vanish with u."""
    x = torch.linspace(-8, 8, 160001, dtype=torch.float64)
    d = R.dgelu64(x)
    assert d.abs().max().item() <= R.GELU_LIP and ((d[1:] - d[:-1]).abs() / (x[1] - x[0])).max().item() <= R.DGELU_LIP
    assert bool((R.gelu_err(x) > 0).all()) and bool((R.dgelu_err(x) > 0).all())
    assert R.gelu_err(x).max().item() < 64 * R.U * 8 and R.dgelu_err(x).max().item() < 64 * R.U


# ------------------------------------------------------------------------------------------------------------------- emulated faults
# fault -> (cases whose check A must break, cases whose bound B must be exceeded); "sin" = the cases with a sinusoid
_ALL = set(W.CASE_IDS)
_SIN = {c.name for c in W.CASES if any(m.sinusoid for m in c.mlps)}
_ODD = {c.name for c in W.CASES if any(m.in_dim % 4 or m.dim % 4 for m in c.mlps)}
_FOLD2 = {c.name for c in W.CASES if max(W.props(c)["fold_passes"]) > 1}
_WIDE = {c.name for c in W.CASES if c.width >= W.FSLAB}
_ROWS = {c.name for c in W.CASES if c.rows > 1}
MUST_CATCH = {
    "last_dropped": (_ALL, _ALL), "tail_dropped": (_ODD, _ODD), "fslab_off_by_one": (_WIDE, _WIDE),
    "bslab_off_by_one": (_ALL, _ALL), "second_fold_dropped": (_FOLD2, _FOLD2), "dgelu_at_h1": (_ALL, _ALL),
    "no_half_at_0": (_ALL, set()), "tanh_gelu": (set(), _ALL), "saved_offset_mlp0": ({"four_mlps"}, {"four_mlps"}),
    "dtable_stride_width": (_ROWS, _ROWS), "sincos_exchanged": (_SIN, _SIN), "freq_half_minus_1": (set(), _SIN),
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_emulated_fault_is_caught(fault):
    """Each fault breaks check A, exceeds bound B, or both, in every case that can show it; the figures are in the module docstring."""
    need_a, need_b = MUST_CATCH[fault]
    assert need_a or need_b
    line = []
    for case in W.CASES:
        ops_a, ref, ops_b = operands(case)
        emu = R.emulate(ops_a, fault)
        broke = sum(int((emu[key].double() != want).sum()) for key, want in ref.items())
        worst, _ = check_b(ops_b, R.emulate(ops_b, fault))
        line.append(f"{case.name} {broke}/{worst:.3g}")
        assert case.name not in need_a or broke > 0, f"{fault}: check A does not see it in {case.name}"
        assert case.name not in need_b or not worst <= 1.0, f"{fault}: bound B does not see it in {case.name} ({worst})"
    print(f"\n  {fault}: " + "  ".join(line))


# ------------------------------------------------------------------------------------------------------------------- refusals
def _descs():
    from vdm4cdm_amd._lib import CondMlp
    mlps = (CondMlp * 4)()
    for k, (in_dim, dim, sin) in enumerate(((64, 128, 1), (6, 64, 0), (5, 65, 0), (8, 8, 0))):
        m = mlps[k]
        m.input, m.in_dim, m.dim, m.sinusoid = 4096, in_dim, dim, sin
        m.w1, m.b1, m.w2, m.b2, m.wproj = 4096, 4096, 4096, 4096, 4096
        m.dw1, m.db1, m.dw2, m.db2, m.dwproj = 8192, 8192, 8192, 8192, 8192
    return mlps


def test_refusals(hip_lib):
    """Fake non-NULL pointers: every call below is refused on the host, before any launch."""
    L = hip_lib
    outs = (C.c_void_p * 4)(8192, 8192, 8192, 8192)

    def fwd(m, n=2, rows=2, width=1312, table=4096):
        return L.vdm_cond_table_fwd(m, n, rows, width, table, None, None)

    def bwd(m, n=2, rows=2, width=1312, stride=1312):
        return L.vdm_cond_table_bwd(m, n, rows, width, 4096, stride, 4096, 4096, None, None)

    def din(m, n=2, rows=2, width=1312):
        return L.vdm_cond_input_grad(m, n, rows, width, 4096, 4096, outs, None)

    calls = (fwd, bwd, din)
    m = _descs()
    for call in calls:
        assert call(m, n=5) != 0 and b"bad arguments" in L.vdm_last_error()
        assert call(m, rows=65536) != 0 and b"65535" in L.vdm_last_error()
    for field in ("in_dim", "dim"):
        m = _descs()
        setattr(m[1], field, 257)
        for call in calls:
            assert call(m) != 0 and b"out of range" in L.vdm_last_error()
    m = _descs()
    m[0].in_dim = 63
    for call in calls:
        assert call(m) != 0 and b"even" in L.vdm_last_error()
    for k, field in ((0, "w1"), (0, "w2"), (1, "wproj")):             # rows of 64, 128 and 64 floats: 16-byte rows
        m = _descs()
        setattr(m[k], field, 4100)
        for call in calls:
            assert call(m) != 0 and b"aligned" in L.vdm_last_error()
    m = _descs()
    m[2].w1, m[2].w2, m[2].wproj = 4100, 4100, 4100                  # rows of 5 and 65 floats: no alignment asked
    m[2].dw1 = None
    assert bwd(m, n=3) != 0 and b"NULL gradient" in L.vdm_last_error()
    m = _descs()
    assert bwd(m, stride=1311) != 0 and b"bad arguments" in L.vdm_last_error()
    for field in ("dw1", "db1", "dw2", "db2", "dwproj"):
        m = _descs()
        setattr(m[1], field, None)
        assert bwd(m) != 0 and b"NULL gradient" in L.vdm_last_error()
    assert fwd(_descs(), table=None) != 0 and b"NULL table" in L.vdm_last_error()
