"""References of the attention kernel checks (csrc/attention.hip), all on the CPU:
  * float64 attention, forward and backward, with the quantities the bounds of check B need;
  * the exact expectations of the one-hot checks A1 / A3 / A4, by index arithmetic alone (no softmax is evaluated);
  * the bounds of check B;
  * an emulation of the three kernels' tile loops in torch fp32 - tiles of 16 (fp32) / 32 (bf16) keys or queries, the -3.0e38 masks, row
    loads clamped to V - 1, column loads of 4-key groups clamped to V - 4, fp32 statistics and accumulators, P and dS rounded to the
    storage type - which reads its transposed operands out of a flat NaN-padded buffer, as the device tests lay them out, so that a
    clamp that leaves the tensor poisons the result here the same way.  `fault` switches one defect on (FAULTS):
    tests/test_attention_cpu.py shows that the healthy emulation passes every check and that each fault fails a check A.
Layouts: q, k, v, dO, gradients [N, H, V, hd]; transposed operands [N, H, hd, V]; lse, dsum [N, H, V]; fp32 tensors hold values already
rounded to the storage type."""
import torch

NEG = -3.0e38
PAD = 64                               # NaN elements on either side of a transposed operand in the emulation
FAULTS = ("no_mask",                   # the ragged tile's `ok` tests removed
          "swap_vt",                   # bf16 forward: the two 16-key sub-tiles swapped on the V^T side only
          "no_rescale",                # forward: o *= alpha removed
          "clamp_v1",                  # col_frag clamps a 4-key group to V - 1 in place of V - 4
          "stats_wrong_head",          # backward: lse and dsum of head h - 1
          "dq_wrong_sample")           # dQ: K^T of sample n - 1

FWD_F32, LSE_TOL = 2e-5, 1e-4
# of max |reference block|, for each of the dQ, dK, dV blocks on its own.  The project's bounds (test_fused_attention_core) are 2e-4 (fp32)
# and 3e-2 (bf16).  bf16 keeps 3e-2 (the MI355X reaches 0.39 of it).  fp32 stayed below 0.1 of 2e-4 on every case - the largest was
# 0.015, dQ of (1, 3, 36, 128) at scores of standard deviation 4 - so it is tightened to 4 x 0.015 x 2e-4 = 1.2e-5.
BWD_TOL = {False: 1.2e-5, True: 3e-2}


def storage(t, bf16):
    return t.bfloat16().float() if bf16 else t


# ------------------------------------------------------------------------------------------------------------------ float64
def ref_forward(q, k, v, scale):
    """-> out [N, H, V, hd], lse [N, H, V], P [N, H, V, V], A = sum_j P_ij |v_jd| (the scale of the forward error bound), float64."""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse[..., None])
    return torch.matmul(P, v), lse, P, torch.matmul(P, v.abs())


def ref_backward(q, k, v, doh, P, scale, dsum):
    """dQ, dK, dV [N, H, V, hd] float64 of out = P v for the upstream gradient doh; dsum [N, H, V] = rowsum(dO * out) (or any tensor
    that stands in for it: the kernels take it as an input)."""
    q, k, v, doh = q.double(), k.double(), v.double(), doh.double()
    dS = P * (torch.matmul(doh, v.transpose(-1, -2)) - dsum.double()[..., None]) * scale
    return torch.matmul(dS, k), torch.matmul(dS.transpose(-1, -2), q), torch.matmul(P.transpose(-1, -2), doh)


def fwd_bound_bf16(A, ref):
    """Per element: twice the first-order worst case of P rounded to bf16 (unit roundoff 2^-8 on every term of sum_j P_ij v_jd, so
    2^-8 A) plus one storage rounding of the result (2^-8 |ref|)."""
    return 2.0 ** -7 * (A + ref.abs()) + 1e-6


def uniform_tol(ref, V, bf16):
    """A2: 0 where V is a power of two (l = V, 1 / V and the product are exact); otherwise one rounding of 1 / V and one of the product,
    2^-22 |ref| with margin for both, and in bf16 one storage rounding on top."""
    if V & (V - 1) == 0:
        return torch.zeros_like(ref)
    return (2.0 ** -22 + (2.0 ** -8 if bf16 else 0.0)) * ref.abs()


# ------------------------------------------------------------------------------------------------------------------ one-hot expectations
def take_rows(x, pi):
    """x [N, H, V, hd], pi [N, H, V] -> x[n, h, pi[n, h, i]]"""
    return torch.gather(x, 2, pi[..., None].expand(x.shape))


def scatter_rows(x, pi):
    """out[n, h, j] = sum of x[n, h, i] over the i with pi[n, h, i] = j (float64)."""
    return torch.zeros_like(x, dtype=torch.float64).scatter_add_(2, pi[..., None].expand(x.shape), x.double())


def onehot_backward(q, k, v, doh, dsum, pi, scale):
    """A3: P is one-hot at pi, so dS[i][pi(i)] = scale (dO_i . v_pi(i) - dsum_i) and every other dS is 0; all integers."""
    ds = scale * ((doh.double() * take_rows(v, pi).double()).sum(-1) - dsum.double())
    dq = ds[..., None] * take_rows(k, pi).double()
    dk = scatter_rows(ds[..., None] * q.double(), pi)
    return dq, dk, scatter_rows(doh, pi)


# ------------------------------------------------------------------------------------------------------------------ emulation
def _rows(x, r0, tk):
    """row_frag: rows r0 .. r0 + tk - 1 of x [N, H, V, hd], clamped to V - 1."""
    idx = torch.clamp(r0 + torch.arange(tk), max=x.shape[2] - 1)
    return x[:, :, idx, :]


def _cols(xt, c0, tk, fault, swap=False):
    """col_frag: for the tk k-slots of one product the columns c0 + s of xt [N, H, hd, V], loaded in groups of 4 that are clamped as a
    group to V - 4 -> [N, H, hd, tk].  Read out of a flat NaN-padded copy: a load that leaves the tensor returns NaN."""
    N, H, hd, V = xt.shape
    s = torch.arange(tk)
    if swap and tk == 32:
        s = (s + 16) % 32
    a0 = c0 + (s // 4) * 4
    a0 = torch.where(a0 + 4 <= V, a0, torch.full_like(a0, V - 1 if fault == "clamp_v1" else V - 4))
    nan = torch.full((PAD,), float("nan"))
    flat = torch.cat([nan, xt.reshape(-1), nan])
    idx = PAD + (torch.arange(N * H * hd) * V)[:, None] + (a0 + s % 4)[None]
    return flat[idx].view(N, H, hd, tk)


def emu_fwd(q, k, vt, scale, bf16, fault=None):
    """attn_fwd_kernel -> out [N, H, V, hd] (rounded to the storage type), lse [N, H, V]."""
    N, H, V, hd = q.shape
    tk = 32 if bf16 else 16
    m, l, o = torch.full((N, H, V), NEG), torch.zeros(N, H, V), torch.zeros(N, H, V, hd)
    for j0 in range(0, V, tk):
        s = torch.matmul(q, _rows(k, j0, tk).transpose(-1, -2))
        ok = (j0 + torch.arange(tk) < V) | (fault == "no_mask")
        s = torch.where(ok, s * scale, torch.full_like(s, NEG))
        mn = torch.maximum(m, s.max(-1).values)
        alpha = torch.exp(m - mn)
        p = torch.exp(s - mn[..., None])
        l = l * alpha + p.sum(-1)
        m = mn
        if fault != "no_rescale":
            o = o * alpha[..., None]
        o = o + torch.matmul(storage(p, bf16), _cols(vt, j0, tk, fault, swap=fault == "swap_vt").transpose(-1, -2))
    return storage(o * (1.0 / l)[..., None], bf16), m + torch.log(l)


def emu_bwd(q, k, v, qt, kt, doh, dot, lse, dsum, scale, bf16, fault=None):
    """attn_bwd_kv_kernel and attn_bwd_q_kernel -> dQ, dK, dV [N, H, V, hd] (rounded to the storage type)."""
    N, H, V, hd = q.shape
    tk = 32 if bf16 else 16
    if fault == "stats_wrong_head":
        lse, dsum = lse.roll(1, 1), dsum.roll(1, 1)
    dk, dv, dq = torch.zeros(N, H, V, hd), torch.zeros(N, H, V, hd), torch.zeros(N, H, V, hd)
    for i0 in range(0, V, tk):                                              # keys as columns, tiles of queries
        i = i0 + torch.arange(tk)
        ok = ((i < V) | (fault == "no_mask"))[:, None]
        ic = torch.clamp(i, max=V - 1)
        s = torch.matmul(_rows(q, i0, tk), k.transpose(-1, -2))
        dp = torch.matmul(_rows(doh, i0, tk), v.transpose(-1, -2))
        pe = torch.where(ok, torch.exp(s * scale - lse[:, :, ic, None]), torch.zeros_like(s))
        ds = pe * (dp - dsum[:, :, ic, None]) * scale
        dv = dv + torch.matmul(storage(pe, bf16).transpose(-1, -2), _cols(dot, i0, tk, fault).transpose(-1, -2))
        dk = dk + torch.matmul(storage(ds, bf16).transpose(-1, -2), _cols(qt, i0, tk, fault).transpose(-1, -2))
    ktq = kt.roll(1, 0) if fault == "dq_wrong_sample" else kt
    for j0 in range(0, V, tk):                                              # queries as columns, tiles of keys
        ok = (j0 + torch.arange(tk) < V) | (fault == "no_mask")
        s = torch.matmul(q, _rows(k, j0, tk).transpose(-1, -2))
        dp = torch.matmul(doh, _rows(v, j0, tk).transpose(-1, -2))
        pe = torch.where(ok, torch.exp(s * scale - lse[..., None]), torch.zeros_like(s))
        ds = pe * (dp - dsum[..., None]) * scale
        dq = dq + torch.matmul(storage(ds, bf16), _cols(ktq, j0, tk, fault).transpose(-1, -2))
    return storage(dq, bf16), storage(dk, bf16), storage(dv, bf16)
