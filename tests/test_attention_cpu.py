"""CPU side of the attention kernel checks (tests/test_attention_kernels_gpu.py):
  * the case table (tests/_attention_cases.py) covers what it is there for - every residue of V mod 32, V below one tile, one ragged
    wave in a second workgroup, every head width with several heads and several samples;
  * the float64 reference (tests/_attention_ref.py) is softmax attention and its autograd gradient;
  * the emulation of the kernels' tile loops passes A1 - A4 exactly and B within its bounds on every case, dtype and scale: the operands
    themselves leave the bounds room (the one-hot scores underflow to exactly 0, the integer sums stay exact, the bf16 rounding of P and
    dS stays inside the forward and backward bounds);
  * each emulated fault (_attention_ref.FAULTS) fails a check A on some case, so the device tests would notice it."""
import pytest
import torch

import _attention_cases as AC
import _attention_ref as R
from _exact import assert_same_bits

BF = {"f32": False, "bf16": True}


def test_case_table_coverage():
    assert AC.coverage_gaps(AC.CASES) == []
    assert AC.ISOLATION_CASE in AC.CASES and AC.ISOLATION_CASE[0] == 2 and AC.ISOLATION_CASE[1] == 3
    n, h, v, hd = AC.ROWDOT_GRID_STRIDE
    assert n * v * h > 4096 * 256 and v % 4 == 0 and v < 2 ** 24
    assert AC.coverage_gaps(AC.CASES[1:]) != [] and AC.coverage_gaps([c for c in AC.CASES if c[2] != 68]) != []      # the checker can fail


def test_reference_is_softmax_attention_and_its_gradient():
    case = (2, 2, 20, 16)
    g = torch.Generator().manual_seed(3)
    q, k, v, do = (torch.randn(case[0], case[1], case[2], case[3], generator=g, dtype=torch.float64) for _ in range(4))
    scale = 0.37
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out_a = torch.matmul(torch.softmax(torch.matmul(leaves[0], leaves[1].transpose(-1, -2)) * scale, -1), leaves[2])
    out_a.backward(do)
    out, lse, P, A = R.ref_forward(q, k, v, scale)
    assert (out - out_a.detach()).abs().max() <= 1e-13
    assert (lse - torch.logsumexp(torch.matmul(q, k.transpose(-1, -2)) * scale, -1)).abs().max() <= 1e-13
    assert (A >= out.abs() - 1e-13).all()
    grads = R.ref_backward(q, k, v, do, P, scale, (do * out).sum(-1))
    for got, leaf in zip(grads, leaves):
        assert (got - leaf.grad).abs().max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- the checks, on the CPU
def transposed(x):
    return x.transpose(-1, -2).contiguous()


def run_onehot(case, bf16, fault=None):
    """A1, A3 and A4 on the emulation; raises AssertionError where a device run would."""
    N, H, V, hd = case
    q, k, pi = AC.onehot_qk(case)
    scale = AC.ONEHOT_SCALE
    # A1
    v = AC.real_values(case, 11, bf16)
    out, lse = R.emu_fwd(q, k, transposed(v), scale, bf16, fault)
    assert_same_bits(out, R.take_rows(v, pi), f"A1 {case}: out")
    assert_same_bits(lse, torch.full((N, H, V), scale * hd), f"A1 {case}: lse")
    # A3
    dout, vi, dsum = AC.onehot_backward_operands(case, bf16)
    doh = AC.to_heads(dout, H)
    ref = R.onehot_backward(q, k, vi, doh, dsum, pi, scale)
    assert max(r.abs().max().item() for r in ref) < 2 ** 24
    lse = torch.full((N, H, V), scale * hd)
    got = R.emu_bwd(q, k, vi, transposed(q), transposed(k), doh, transposed(doh), lse, dsum, scale, bf16, fault)
    for name, g_, r_ in zip(("dQ", "dK", "dV"), got, ref):
        assert_same_bits(g_, R.storage(r_.float(), bf16), f"A3 {case}: {name}")
    # A4
    outi, _ = R.emu_fwd(q, k, transposed(vi), scale, bf16, fault)
    dsum4 = (doh * outi).sum(-1)
    got = R.emu_bwd(q, k, vi, transposed(q), transposed(k), doh, transposed(doh), lse, dsum4, scale, bf16, fault)
    assert_same_bits(got[0], torch.zeros_like(got[0]), f"A4 {case}: dQ")
    assert_same_bits(got[1], torch.zeros_like(got[1]), f"A4 {case}: dK")
    assert_same_bits(got[2], R.storage(ref[2].float(), bf16), f"A4 {case}: dV")


def run_uniform(case, bf16, fault=None):
    """A2 on the emulation."""
    N, H, V, hd = case
    k, v = AC.real_values(case, 12, bf16), AC.int_values(case, 13)
    out, lse = R.emu_fwd(torch.zeros(N, H, V, hd), k, transposed(v), 1.0, bf16, fault)
    ref = v.double().sum(2, keepdim=True).expand(N, H, V, hd) / V
    if V & (V - 1) == 0:
        assert_same_bits(out, R.storage(ref.float(), bf16), f"A2 {case}: out")
    else:
        assert ((out.double() - ref).abs() <= R.uniform_tol(ref, V, bf16)).all(), f"A2 {case}: out"


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("case", AC.CASES, ids=AC.IDS)
def test_emulation_passes_the_exact_checks(case, dtype):
    run_onehot(case, BF[dtype])
    run_uniform(case, BF[dtype])


def b_ratios(case, bf16, scale, fault=None):
    """Check B on the emulation -> {quantity: max err / bound}."""
    N, H, V, hd = case
    q, k, v, dout = AC.b_operands(case, bf16)
    doh = AC.to_heads(dout, H)
    ref, rlse, P, A = R.ref_forward(q, k, v, scale)
    out, lse = R.emu_fwd(q, k, transposed(v), scale, bf16, fault)
    err = (out.double() - ref).abs()
    r = {"out": (err / R.fwd_bound_bf16(A, ref)).max().item() if bf16 else err.max().item() / (R.FWD_F32 * ref.abs().max().item()),
         "lse": (lse.double() - rlse).abs().max().item() / R.LSE_TOL}
    dsum = (doh * out).sum(-1)
    grads = R.emu_bwd(q, k, v, transposed(q), transposed(k), doh, transposed(doh), lse, dsum, scale, bf16, fault)
    for name, g_, r_ in zip(("dQ", "dK", "dV"), grads, R.ref_backward(q, k, v, doh, P, scale, (doh.double() * ref).sum(-1))):
        r[name] = (g_.double() - r_).abs().max().item() / (R.BWD_TOL[bf16] * r_.abs().max().item())
    return r


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("case", AC.CASES, ids=AC.IDS)
def test_emulation_is_inside_the_bounds_of_check_b(case, dtype):
    for name, scale in AC.b_scales(case[3]):
        r = b_ratios(case, BF[dtype], scale)
        print(f"{case} {dtype} {name}: err / bound " + "  ".join(f"{k} {x:.3f}" for k, x in r.items()))
        assert all(x <= 1.0 for x in r.values()), (case, dtype, name, r)


# ---------------------------------------------------------------------------------------------------------------- teeth
@pytest.mark.parametrize("fault", R.FAULTS)
def test_each_emulated_fault_fails_an_exact_check(fault):
    caught = []
    for case in AC.CASES:
        for dtype in AC.DTYPES:
            for run in (run_onehot, run_uniform):
                try:
                    run(case, BF[dtype], fault)
                except AssertionError:
                    caught.append((case, dtype, run.__name__))
        if len(caught) >= 2:
            break
    print(fault, "caught by", caught)
    assert caught, f"no check A notices the emulated fault {fault}"


def test_lse_of_the_wrong_head_is_outside_check_b():
    """The one-hot lse is the same number in every head, so check A cannot tell the heads' lse apart (it does tell their dsum apart, which
    the emulated fault above swaps as well); with random reals the heads' lse differ and the backward bound of B notices."""
    case, bf16 = (1, 2, 12, 32), False
    N, H, V, hd = case
    scale = hd ** -0.5
    q, k, v, dout = AC.b_operands(case, bf16)
    doh = AC.to_heads(dout, H)
    ref, rlse, P, _ = R.ref_forward(q, k, v, scale)
    out, lse = R.emu_fwd(q, k, transposed(v), scale, bf16)
    dsum = (doh * out).sum(-1)
    grads = R.emu_bwd(q, k, v, transposed(q), transposed(k), doh, transposed(doh), lse.roll(1, 1), dsum, scale, bf16)
    refs = R.ref_backward(q, k, v, doh, P, scale, (doh.double() * ref).sum(-1))
    assert any((g_.double() - r_).abs().max().item() > R.BWD_TOL[bf16] * r_.abs().max().item() for g_, r_ in zip(grads, refs))
