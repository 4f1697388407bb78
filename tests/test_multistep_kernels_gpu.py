"""vdm_multistep_step (K9m) on the GPU: exact-integer parity (independent of any fma contraction), a float64 comparison under a bound
derived from the roundings the header spells out (tests/_multistep_ref.py step64; no measured constant), and the history contract - a
row with w_p == 0 never reads prev, prev always receives the estimate, nothing past n is touched.  Sizes: ANCESTRAL_NS of _step_cases
(tails of 1 / 2 / 3, one group + 1, 255 groups + 3, more groups than one sweep of the grid + 2), rows 0 and 3 of a 5-row table."""
import pytest
import torch

import _multistep_cases as C
import _multistep_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _table(first, second):
    """5 rows: rows 0 and 4 first order (`first`), rows 1..3 `second`; fp32 on the device, [5, 8]."""
    rows = [list(first) + [0.25, 0, 0]] + [list(second) + [0.5, 0, 0]] * 3 + [list(first) + [0.75, 0, 0]]
    return torch.tensor(rows, dtype=torch.float32)


def _launch(z, eh, prev, coef, row, eu=None, w=0.0, n=None):
    """One launch on the first n elements of (padded) device copies; returns (z, prev) on the host, padding included."""
    from vdm4cdm_amd import _lib, hip_ops as ops
    zd, pd, hd = z.to(DEV), prev.to(DEV), eh.to(DEV)
    ud = None if eu is None else eu.to(DEV)
    step = torch.tensor([row], dtype=torch.int32, device=DEV)
    cd = coef.to(DEV)
    if n is None:
        ops.multistep_step(zd, hd, pd, cd, step, eps_uncond=ud, w_cfg=w)
    else:
        _lib.check(_lib.lib().vdm_multistep_step(zd.data_ptr(), hd.data_ptr(), None if ud is None else ud.data_ptr(), float(w), pd.data_ptr(),
                                                 cd.data_ptr(), step.data_ptr(), n, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert int(step.item()) == row                           # the kernel reads the counter, it does not advance it
    return zd.cpu(), pd.cpu()


def _even_ints(n, seed, lo=-4, hi=5):
    return (2 * torch.randint(lo, hi, (n,), generator=torch.Generator().manual_seed(seed))).to(torch.int64)


# ------------------------------------------------------------------------------ 8. exact
@pytest.mark.parametrize("n", C.KERNEL_NS)
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
def test_multistep_step_is_exact_on_integers(n, cfg):
    """Even-integer fields in [-8, 8], coefficients that are powers of two or small integers, w_cfg = 0.5: every product and sum is an
    integer below 2^24, so z and prev equal the int64 result bit for bit whatever the compiler fused."""
    coef = _table(C.EXACT_ROW_FIRST, C.EXACT_ROW_SECOND)
    z, eh, eu, prev = (_even_ints(n, 10 + k) for k in range(4))
    for row in C.KERNEL_ROWS:
        e_z, e_e, w_z, w_x, w_p = (float(v) for v in coef[row, :5])
        e2 = 3 * eh - eu if cfg else 2 * eh                  # twice the (blended) network output: (1 + w) eh - w eu at w = 1/2
        est = (int(2 * e_z) * z + int(e_e) * e2) // 2
        assert torch.equal(2 * est, int(2 * e_z) * z + int(e_e) * e2)
        zn = (int(2 * w_z) * z) // 2 + int(w_x) * est + int(w_p) * prev
        got_z, got_p = _launch(z.float(), eh.float(), prev.float(), coef, row, eu.float() if cfg else None, C.EXACT_W_CFG if cfg else 0.0)
        assert torch.equal(got_z, zn.float()) and torch.equal(got_p, est.float()), f"row {row}"
        assert (w_p != 0.0) == (row == 3)


# ------------------------------------------------------------------------------ 9. float64 bound
def _real_case(n, seed):
    g = torch.Generator().manual_seed(seed)
    z, eh, eu, prev = (torch.randn(n, generator=g) for _ in range(4))
    tab = R.as_table(R.vdm_rows(C.KERNEL_TABLE_ROWS, 2, True)).float()        # the real coefficients of a 5-step dpm2m chain, as fp32
    return 3.0 * z, eh, eu, 2.0 * prev, tab


@pytest.mark.parametrize("n", C.KERNEL_NS)
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
def test_multistep_step_within_the_derived_bound_of_float64(n, cfg):
    """Real inputs and the real coefficients of a 5-step chain: |device - float64| <= the bound of step64 element by element, for z and
    for prev.  The bound is tight enough to matter: the float64 result of the table with w_x and w_p exchanged lies outside it."""
    z, eh, eu, prev, tab = _real_case(n, 77)
    w = float(torch.tensor(C.W_CFG, dtype=torch.float32))
    d = lambda a: a.double()
    for row in C.KERNEL_ROWS:
        got_z, got_p = _launch(z, eh, prev, tab, row, eu if cfg else None, w if cfg else 0.0)
        coefs = [float(v) for v in tab[row, :5].double()]
        ref_z, ref_p, b_z, b_p = R.step64(d(z), d(eh), d(eu) if cfg else None, w, d(prev), coefs)
        err_z, err_p = (d(got_z) - ref_z).abs(), (d(got_p) - ref_p).abs()
        print(f"n={n} row={row} cfg={cfg}: max err z {err_z.max().item():.3e} (bound {b_z.max().item():.3e}), "
              f"prev {err_p.max().item():.3e} (bound {b_p.max().item():.3e})")
        assert (err_z <= b_z).all() and (err_p <= b_p).all(), f"row {row}"
        if row == 3:
            swapped = coefs[:3] + [coefs[4], coefs[3]]
            bad_z = R.step64(d(z), d(eh), d(eu) if cfg else None, w, d(prev), swapped)[0]
            assert ((d(got_z) - bad_z).abs() > b_z).any(), "the bound would not notice w_x and w_p exchanged"
            assert tab[row, 4].item() != 0.0
        else:
            assert tab[row, 4].item() == 0.0


# ------------------------------------------------------------------------------ 10. history
@pytest.mark.parametrize("n", C.KERNEL_NS)
def test_history_contract(n):
    z, eh, _, prev, tab = _real_case(n, 91)
    pad = lambda a: torch.cat([a, torch.full((C.PAD,), C.SENTINEL)])
    # a row with w_p == 0 does not read prev: NaN history, finite z that is the two-term result, prev <- est
    nan_prev = torch.full((n,), float("nan"))
    got_z, got_p = _launch(pad(z), pad(eh), pad(nan_prev), tab, 0, n=n)
    clean_z, clean_p = _launch(z, eh, torch.zeros(n), tab, 0)
    assert torch.isfinite(got_z[:n]).all() and torch.equal(got_z[:n], clean_z)
    assert torch.isfinite(got_p[:n]).all() and torch.equal(got_p[:n], clean_p)
    coefs = [float(v) for v in tab[0, :5].double()]
    ref_z, ref_p, b_z, b_p = R.step64(z.double(), eh.double(), None, 0.0, None, coefs)
    assert ((got_z[:n].double() - ref_z).abs() <= b_z).all() and ((got_p[:n].double() - ref_p).abs() <= b_p).all()
    # nothing past n is written, in z or in prev
    assert (got_z[n:] == C.SENTINEL).all() and (got_p[n:] == C.SENTINEL).all()
    # a row with w_p != 0 reads it: another prev, another z (and the same est)
    a_z, a_p = _launch(pad(z), pad(eh), pad(prev), tab, 3, n=n)
    b_z2, b_p2 = _launch(pad(z), pad(eh), pad(prev + 1.0), tab, 3, n=n)
    assert not torch.equal(a_z[:n], b_z2[:n]) and (a_z[:n] != b_z2[:n]).all() and torch.equal(a_p[:n], b_p2[:n])
    assert (a_z[n:] == C.SENTINEL).all() and (a_p[n:] == C.SENTINEL).all()


def test_unaligned_fields_take_the_scalar_path():
    """Fields that start 4 bytes into an allocation are not 16-byte aligned: the entry point sends every element through the tail loop;
    the same bits as the aligned launch."""
    from vdm4cdm_amd import _lib
    n = 1023
    z, eh, _, prev, tab = _real_case(n, 5)
    want_z, want_p = _launch(z, eh, prev, tab, 3)
    off = lambda a: torch.cat([torch.full((1,), C.SENTINEL), a, torch.full((C.PAD,), C.SENTINEL)]).to(DEV)
    zd, hd, pd, cd = off(z), off(eh), off(prev), tab.to(DEV)
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().vdm_multistep_step(zd.data_ptr() + 4, hd.data_ptr() + 4, None, 0.0, pd.data_ptr() + 4, cd.data_ptr(), step.data_ptr(),
                                             n, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(zd[1:n + 1].cpu(), want_z) and torch.equal(pd[1:n + 1].cpu(), want_p)
    for a in (zd, pd):
        assert a[0].item() == C.SENTINEL and (a[n + 1:] == C.SENTINEL).all()
