"""CPU side of the forward / input-gradient conv kernel checks (tests/test_conv_kernels_gpu.py):
  * ref_fwd / ref_dgrad (tests/_conv_ref.py: plain shifted matrix products and their explicit transpose) ARE F.conv3d and its input
    gradient: bit-equal to float64 autograd on integer operands (both sums are then exact, so any difference is an indexing
    difference) and to 1e-13 on random reals, in every mode - zeros, circular, stride 2, up-sampling, ksize 1, circular grids smaller
    than the halo; on integers a float32 evaluation of the same sums has the same bits (every partial sum is an integer below 2^24);
  * every case of the table (tests/_conv_cases.py) reaches the kernel, tile and segmenting it names (vdm_conv_plan is host only), the
    new query agrees with the four older ones, and the table covers everything plan_of() can pick;
  * the derived bound of check B is measured against the reference, never a kernel: an fp32 emulation of each kernel's summation
    order (K-blocks, taps, the K-split fold, the classes with their merged and re-rounded weights, the epilogue, the store) lies inside
    it, and four emulated faults lie outside - one dropped tap on one tile face, one zero-padded voxel read as wrapped, one channel of
    a partial K-block read from the padding, one class entry with a wrong merged tap."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _conv_cases as W
import _conv_ref as R
from _exact import assert_same_bits, ints, ints_biased


# ------------------------------------------------------------------------------------------------------- the reference is conv3d
def autograd_conv(x, w, ks, stride, ups, circular, dout=None, dtype=torch.float64):
    """F.conv3d of the same conv in the channels-last layout; with dout its input gradient by autograd."""
    xl = x.to(dtype).clone().requires_grad_(dout is not None)
    xc = xl.permute(0, 4, 1, 2, 3)
    if ups:
        xc = F.interpolate(xc, scale_factor=2, mode="nearest")
    cout, cin, pad = w.shape[1], w.shape[2], ks // 2
    wc = w.to(dtype).reshape(ks, ks, ks, cout, cin).permute(3, 4, 0, 1, 2)
    if pad and circular:
        y = F.conv3d(F.pad(xc, (pad,) * 6, mode="circular"), wc, stride=stride)
    else:
        y = F.conv3d(xc, wc, stride=stride, padding=pad)
    y = y.permute(0, 2, 3, 4, 1)
    if dout is None:
        return y.detach()
    y.backward(dout.to(dtype))
    return xl.grad


# name, N, output grid, cin, cout, ks, stride, ups, circular
REF_MODES = [
    ("zeros", 2, (3, 5, 7), 3, 5, 3, 1, 0, False),
    ("circular", 2, (3, 5, 7), 3, 5, 3, 1, 0, True),
    ("circular_1x1x1", 1, (1, 1, 1), 4, 3, 3, 1, 0, True),
    ("circular_2x4x6", 1, (2, 4, 6), 4, 3, 3, 1, 0, True),
    ("stride2", 2, (2, 3, 5), 3, 4, 3, 2, 0, False),
    ("stride2_circular", 1, (1, 1, 2), 3, 4, 3, 2, 0, True),
    ("ups", 1, (4, 6, 10), 3, 4, 3, 1, 1, False),
    ("ups_circular", 2, (2, 2, 2), 3, 4, 3, 1, 1, True),
    ("ksize1", 2, (3, 5, 7), 5, 3, 1, 1, 0, False),
]


@pytest.mark.parametrize("mode", REF_MODES, ids=[m[0] for m in REF_MODES])
def test_ref_is_conv3d_and_its_autograd(mode):
    name, n, grid, cin, cout, ks, stride, ups, circ = mode
    ish = R.input_shape(n, grid, stride, ups)
    nt = ks ** 3 * max(cin, cout) * 8
    for mk in (ints, ints_biased):
        x, dout, w = mk(ish + (cin,), 1, nt), mk((n,) + grid + (cout,), 2, nt), mk((ks ** 3, cout, cin), 3, nt)
        out, abs_sum = R.ref_fwd(x, w, ks, stride, ups, circ)
        assert_same_bits(out, autograd_conv(x, w, ks, stride, ups, circ), f"{name}: ref_fwd vs float64 conv3d")
        assert_same_bits(abs_sum, autograd_conv(x.abs(), w.abs(), ks, stride, ups, circ), f"{name}: ref_fwd abs_sum")
        dx, dabs = R.ref_dgrad(dout, w, ks, stride, ups, circ)
        assert_same_bits(dx, autograd_conv(x, w, ks, stride, ups, circ, dout), f"{name}: ref_dgrad vs float64 autograd")
        assert_same_bits(dabs, autograd_conv(x, w.abs(), ks, stride, ups, circ, dout.abs()), f"{name}: ref_dgrad abs_sum")
    g = torch.Generator().manual_seed(3)
    x, dout, w = (torch.randn(s, generator=g, dtype=torch.float64) for s in (ish + (cin,), (n,) + grid + (cout,), (ks ** 3, cout, cin)))
    out, abs_sum = R.ref_fwd(x, w, ks, stride, ups, circ)
    assert ((out - autograd_conv(x, w, ks, stride, ups, circ)).abs() <= 1e-13 * abs_sum + 1e-300).all()
    dx, dabs = R.ref_dgrad(dout, w, ks, stride, ups, circ)
    assert ((dx - autograd_conv(x, w, ks, stride, ups, circ, dout)).abs() <= 1e-13 * dabs + 1e-300).all()


def test_ref_epilogue_terms():
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn((2, 3, 4, 5, 3), generator=g), torch.randn((27, 4, 3), generator=g)
    bias, nbias, res = torch.randn(4, generator=g), torch.randn((2, 4), generator=g), torch.randn((2, 3, 4, 5, 4), generator=g)
    out, a = R.ref_fwd(x, w, 3, 1, 0, False)
    full, fa = R.ref_fwd(x, w, 3, 1, 0, False, bias=bias, nbias=nbias, res=res)
    assert torch.equal(full, out + bias.double() + nbias.double()[:, None, None, None, :] + res.double())
    assert torch.equal(fa, a + bias.double().abs() + nbias.double().abs()[:, None, None, None, :] + res.double().abs())
    assert R.ref_fwd(x, w, 3, 1, 0, False, want_abs=False)[1] is None


@pytest.mark.parametrize("name", ["g_2x8_fwd", "ups_64_32_circ_dgrad"])
def test_fp32_reference_has_the_float64_bits_on_integers(name):
    """What lets check A evaluate its largest references in float32: every partial sum is an integer below 2^24."""
    c = W.BY_NAME[name]
    for mk in (ints, ints_biased):
        xin, w = mk(W.in_shape(c), 11, W.terms(c)), mk((c.ks ** 3, c.cout, c.cin), 12, W.terms(c))
        bias, nbias, res = W.epilogue_operands(c, 13, real=False)
        r64 = W.ref(c, xin, w, bias, nbias, res, want_abs=False)[0]
        r32 = W.ref(c, xin, w, bias, nbias, res, dtype=torch.float32, want_abs=False)[0]
        assert r32.dtype == torch.float32 and r64.abs().max().item() < 2 ** 24
        assert_same_bits(r32, r64, f"{name}: float32 reference vs float64")


# ------------------------------------------------------------------------------------------------------------------- the plans
@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_case_reaches_its_kernel(case):
    from vdm4cdm_amd import _lib
    L = _lib.lib()
    d, info = W.plan_of(case)
    W.assert_plan(case, info)
    dgrad = int(case.direction == "dgrad")
    # the new query against the four older ones
    assert info.family == L.vdm_conv_kernel_variant(d, dgrad)
    assert info.packed_bytes == L.vdm_conv_packed_bytes(d, dgrad) and info.packed_bytes > 0
    if dgrad:
        plain = case.ks == 3 and case.stride == 1 and not case.ups
        assert L.vdm_conv_dgrad_gn_tiles(d) == (info.tiles if plain else 0)
    else:
        assert info.tiles == L.vdm_conv_gn_tiles(d)
    item = _lib.PackItem()
    assert L.vdm_conv_pack_plan(d, dgrad, ctypes.c_void_p(64), ctypes.c_void_p(64), ctypes.byref(item)) == 0
    assert (item.variant, item.cls_kind, item.nc, item.nchunks, item.nkb) == (info.layout, info.cls_kind, info.nc, info.nchunks, info.nkb)
    assert item.elems * (2 if case.dtype == W.BF else 4) == info.packed_bytes
    # the launch grid from the plan's own fields
    n, (Dz, Dy, Dx) = case.n, (tuple(g // 2 for g in case.grid) if case.ups else case.grid)
    fam, kind = W.family_of(info), W.cls_kind_of(info)
    cols = R.cdiv(Dy, info.ty) * R.cdiv(Dx, 16)
    spatial = cols * (info.nseg if info.roll else R.cdiv(Dz, info.tz))
    mult = 2 if fam == "SPLIT" else (8 if fam == "CLASS" and kind != "UP_DGRAD" else 1)
    assert info.workgroups == n * info.nchunks * spatial * mult
    assert info.tiles == cols * R.cdiv(Dz, info.tz) * (8 if kind == "UP_FWD" else 1)
    if info.roll:
        ntz = R.cdiv(Dz, 4)
        assert (info.tz, info.ty) == (4, 8) and info.nseg == R.cdiv(ntz, info.zsteps) and info.zsteps >= 2
    else:
        assert info.nseg == 0 and info.zsteps == 0
    L_ = W.depth(case, info, False)
    assert 8 < L_ < 1000


def test_case_table_covers_the_plan():
    plans = {c.name: W.plan_of(c)[1] for c in W.CASES}
    fam = lambda c: W.family_of(plans[c.name])                                       # noqa: E731
    assert {fam(c) for c in W.CASES} == set(W.FAMILIES)
    by = lambda f: [c for c in W.CASES if fam(c) == f]                               # noqa: E731
    assert {plans[c.name].nc for c in by("KPACK")} == {1, 2} and {c.direction for c in by("KPACK")} == {"fwd", "dgrad"}
    assert {plans[c.name].ty for c in by("KSPLIT")} == {4, 8} and all(plans[c.name].tz == 1 for c in by("KSPLIT"))
    assert max(plans[c.name].nkb for c in by("KSPLIT")) == 8 and any(plans[c.name].nkb % 4 for c in by("KSPLIT"))
    # every (tz, ty) the generic and SPLIT launchers build; rolling and not; equal and unequal segments
    ks3 = [c for c in by("GENERIC") if c.ks == 3 and c.stride == 1]
    for nc in (1, 2, 4):
        want = {(1, 4), (1, 8), (2, 8), (4, 8)} if nc > 1 else {(1, 4)}
        got = {(plans[c.name].tz, plans[c.name].ty) for c in ks3 if plans[c.name].nc == nc and c.dtype == W.BF}
        assert want <= got, f"generic NC{nc}: tiles {sorted(got)}"
    assert {(plans[c.name].tz, plans[c.name].ty) for c in by("SPLIT")} == {(1, 4), (1, 8), (2, 8)}
    assert {(plans[c.name].tz, plans[c.name].ty) for c in W.CASES if c.stride == 2 and c.direction == "fwd"} == {(2, 4)}
    rolls = [c for c in ks3 if plans[c.name].roll]
    assert {c.direction for c in rolls} == {"fwd", "dgrad"} and {c.circ for c in rolls} == {False, True}
    assert any(plans[c.name].tz == 4 and not plans[c.name].roll for c in ks3)
    seg = lambda c: (R.cdiv(c.grid[0], 4), plans[c.name].nseg, plans[c.name].zsteps)  # noqa: E731
    assert any(ntz == ns * zs for ntz, ns, zs in map(seg, rolls)) and any(ntz < ns * zs for ntz, ns, zs in map(seg, rolls))
    assert any(W.K(c) % 32 for c in rolls)
    # all three class kinds at every NC launch_cls switches over
    kinds = {(W.cls_kind_of(plans[c.name]), plans[c.name].nc) for c in by("CLASS") if c.dtype == W.BF}
    assert kinds == {(k, nc) for k in W.CLS_KINDS for nc in (1, 2, 4)}
    assert {W.cls_kind_of(plans[c.name]) for c in by("CLASS") if c.dtype == W.F32} == set(W.CLS_KINDS)
    # both storage types, the fp32 output, ksize 1, both paddings in every family, partial chunks and K-blocks
    assert {c.dtype for c in W.CASES} == {W.BF, W.F32} and any(c.out_f32 for c in W.CASES)
    assert {c.dtype for c in W.CASES if c.ks == 1} == {W.BF, W.F32}
    for f in W.FAMILIES:
        if f != "SPLIT":
            assert {c.circ for c in by(f)} == {False, True}, f
    assert any(W.O(c) % (16 * plans[c.name].nc) for c in by("GENERIC")) and any(W.K(c) % 32 for c in by("GENERIC") if c.dtype == W.BF)
    assert any(W.K(c) % 16 for c in W.CASES if c.dtype == W.F32)
    assert max(c.n * c.grid[0] * c.grid[1] * c.grid[2] for c in W.CASES) <= 140_000
    # check B: every family, every class kind, every generic tile, rolling, both storage types; the partials run once per family
    b = [W.BY_NAME[n] for n in W.B_CASES]
    assert {fam(c) for c in b} == set(W.FAMILIES)
    assert {(W.cls_kind_of(plans[c.name]), c.dtype) for c in b if fam(c) == "CLASS"} == {(k, t) for k in W.CLS_KINDS for t in (W.BF, W.F32)}
    assert {(plans[c.name].tz, plans[c.name].ty) for c in b if fam(c) in ("GENERIC", "SPLIT")} >= {(1, 4), (1, 8), (2, 8), (4, 8), (2, 4)}
    assert any(plans[c.name].roll for c in b) and {plans[c.name].ty for c in b if fam(c) == "KSPLIT"} == {4, 8}
    gn = [W.BY_NAME[n] for n in W.GN_CASES]
    assert all(c.direction == "fwd" for c in gn) and {fam(c) for c in gn} == set(W.FAMILIES) and any(plans[c.name].roll for c in gn)


def test_plan_query_reports_the_refusals():
    """The descriptor-level refusals of vdm_conv_fwd come back from the host-only query, a dgrad ignores out_f32, bad arguments fail."""
    from vdm4cdm_amd import _lib
    L = _lib.lib()
    info = _lib.ConvPlanInfo()
    ok = W.BY_NAME["g_conv_out_f32_fwd"]
    for what, kw in (("cout 32", dict(cout=32)), ("ksize 1", dict(ks=1)), ("stride 2", dict(stride=2)), ("upsample", dict(ups=1, grid=(6, 10, 18)))):
        c = ok._replace(**kw)
        assert L.vdm_conv_plan(W.desc_of(c), 0, ctypes.byref(info)) != 0, what
        assert b"out_f32" in L.vdm_last_error() or b"fp32 output" in L.vdm_last_error()
        assert L.vdm_conv_plan(W.desc_of(c), 1, ctypes.byref(info)) == 0, what
    assert L.vdm_conv_plan(W.desc_of(ok._replace(dtype=W.F32, cout=32)), 0, ctypes.byref(info)) == 0      # fp32 storage stores fp32 anyway
    assert L.vdm_conv_plan(W.desc_of(ok), 0, None) != 0
    assert L.vdm_conv_plan(None, 0, ctypes.byref(info)) != 0
    assert L.vdm_conv_plan(W.desc_of(ok._replace(ks=2)), 0, ctypes.byref(info)) != 0


# ---------------------------------------------------------------------------------------------------------------- check B, CPU half
def _round(t, dtype):
    return t.to(dtype).float()


def _fwd_view(c, xin, w):
    """A non-class launch as the kernel sees it: a forward conv of the staged tensor S with weights Wk[t] [O, K]; a dgrad is the
    stride-1 conv of dout with the flipped, transposed taps."""
    if c.direction == "dgrad":
        return xin, torch.flip(w, dims=(0,)).transpose(1, 2).contiguous(), 1
    if c.ups:
        for axis in (1, 2, 3):
            xin = xin.repeat_interleave(2, dim=axis)
    return xin, w, c.stride


def _shifted(Sp, t, ks, stride, D, H, Wd):
    dz, dy, dx = t // (ks * ks), (t // ks) % ks, t % ks
    return Sp[:, dz:dz + stride * D:stride, dy:dy + stride * H:stride, dx:dx + stride * Wd:stride]


def emulate(c, info, xin, w, bias, nbias, res):
    """The launch in torch fp32 in the kernel's summation order (the accumulator before the store, fp32, in the output's shape)."""
    fam, kind = W.family_of(info), W.cls_kind_of(info)
    KB = 32 if c.dtype == W.BF else 16
    n = c.n
    if fam != "CLASS":
        S, Wk, stride = _fwd_view(c, xin.float(), w.float())
        D, H, Wd = (s // stride for s in S.shape[1:4])
        Sp = R._padded(S, c.ks // 2, c.circ)
        O, K, T = Wk.shape[1], Wk.shape[2], c.ks ** 3
        nwave = 4 if fam == "KSPLIT" else 1
        acc = [torch.zeros((n * D * H * Wd, O)) for _ in range(nwave)]
        if fam == "KPACK":
            for g in range(7):                               # 4 taps x 8 channels per MFMA
                taps = [t for t in range(4 * g, 4 * g + 4) if t < 27]
                xs = torch.cat([_shifted(Sp, t, 3, 1, D, H, Wd).reshape(-1, K) for t in taps], dim=1)
                acc[0] += xs @ torch.cat([Wk[t] for t in taps], dim=1).t()
        else:
            for kb in range(info.nkb):
                k0, k1 = kb * KB, min(K, kb * KB + KB)
                for t in range(T):
                    acc[kb % nwave] += _shifted(Sp, t, c.ks, stride, D, H, Wd)[..., k0:k1].reshape(-1, k1 - k0) @ Wk[t][:, k0:k1].t()
        tot = (acc[0] + acc[1]) + (acc[2] + acc[3]) if nwave == 4 else acc[0]
        tot = tot.view(n, D, H, Wd, O)
    else:
        cd, ch, cw = (g // 2 for g in c.grid) if c.ups else c.grid
        mode_b = kind == "UP_DGRAD"
        K, O = W.K(c), W.O(c)
        src = xin.float()
        fine = torch.zeros((n, 2 * cd, 2 * ch, 2 * cw, O))
        coarse = torch.zeros((n * cd * ch * cw, O))
        for cl in range(8):
            pz, py, px = (cl >> 2) & 1, (cl >> 1) & 1, cl & 1
            Sp = R._padded(src[:, pz::2, py::2, px::2] if mode_b else src, 1, c.circ)
            acc = coarse if mode_b else torch.zeros((n * cd * ch * cw, O))
            for (oz, oy, ox), taps in R.cls_entries(kind, cl):
                Wm = torch.zeros((c.cout, c.cin))
                for t in taps:                               # pack_value: ascending master taps in fp32, then the storage type
                    Wm = Wm + w.float()[t]
                Wm = _round(Wm, c.dtype)
                if c.direction == "dgrad":
                    Wm = Wm.t()
                sz, sy, sx = ((1 - oz, 1 - oy, 1 - ox) if mode_b else (1 + oz, 1 + oy, 1 + ox))
                xs = Sp[:, sz:sz + cd, sy:sy + ch, sx:sx + cw].reshape(-1, K)
                for kb in range(info.nkb):
                    k0, k1 = kb * KB, min(K, kb * KB + KB)
                    acc += xs[:, k0:k1] @ Wm[:, k0:k1].t()
            if not mode_b:
                fine[:, pz::2, py::2, px::2] = acc.view(n, cd, ch, cw, O)
        tot = coarse.view(n, cd, ch, cw, O) if mode_b else fine
    if bias is not None or nbias is not None:
        badd = (bias.float() if bias is not None else torch.zeros(1))
        if nbias is not None:
            badd = badd + nbias.float()[:, None, None, None, :]
        tot = tot + badd
    if res is not None:
        tot = tot + res.float()
    return tot


def _store(t, c):
    return t.to(W.out_dtype(c)).double()


def _faults(c, info, xin, w):
    """(name, delta) of the emulated faults that apply to the case: delta is the change of the output, in float64."""
    fam, kind = W.family_of(info), W.cls_kind_of(info)
    xin, w = xin.double(), w.double()
    out = []
    if fam == "CLASS":
        # one class entry with a wrong merged tap: class 7, entry 0 lacks its last master tap (stride-2 dgrad: takes the next tap instead)
        cd, ch, cw = (g // 2 for g in c.grid) if c.ups else c.grid
        mode_b = kind == "UP_DGRAD"
        (oz, oy, ox), taps = R.cls_entries(kind, 7)[0]
        dW = (w[(taps[-1] + 1) % 27] - w[taps[-1]]) if kind == "S2_DGRAD" else -w[taps[-1]]
        if c.direction == "dgrad":
            dW = dW.t()
        Sp = R._padded(xin[:, 1::2, 1::2, 1::2] if mode_b else xin, 1, c.circ)
        sz, sy, sx = ((1 - oz, 1 - oy, 1 - ox) if mode_b else (1 + oz, 1 + oy, 1 + ox))
        d = (Sp[:, sz:sz + cd, sy:sy + ch, sx:sx + cw].reshape(-1, W.K(c)) @ dW.t()).view(c.n, cd, ch, cw, W.O(c))
        delta = torch.zeros(W.out_shape(c), dtype=torch.float64)
        if mode_b:
            delta += d
        else:
            delta[:, 1::2, 1::2, 1::2] = d
        return [("wrong merged tap", delta)]
    S, Wk, stride = _fwd_view(c, xin, w)
    D, H, Wd = (s // stride for s in S.shape[1:4])
    pad, T, K = c.ks // 2, c.ks ** 3, Wk.shape[2]
    Sp = R._padded(S, pad, c.circ)
    # 1. the last tap dropped on the x face of the first tile column
    face = min(15, Wd - 1)
    delta = torch.zeros(W.out_shape(c), dtype=torch.float64)
    delta[:, :, :, face] = -(_shifted(Sp, T - 1, c.ks, stride, D, H, Wd)[:, :, :, face] @ Wk[T - 1].t())
    out.append(("dropped tap on a tile face", delta))

    def one_voxel(pos, value):
        """delta when the padded-grid voxel `pos` of sample 0 carries `value` [K] more than it should."""
        delta = torch.zeros(W.out_shape(c), dtype=torch.float64)
        for t in range(T):
            tt = (t // (c.ks * c.ks), (t // c.ks) % c.ks, t % c.ks)
            v = [(p - d) for p, d in zip(pos, tt)]
            if all(q % stride == 0 and 0 <= q // stride < lim for q, lim in zip(v, (D, H, Wd))):
                delta[0, v[0] // stride, v[1] // stride, v[2] // stride] += Wk[t] @ value
        return delta
    # 2. the zero-padded voxel (-1, 0, 0) of sample 0 read as wrapped
    if pad and not c.circ:
        out.append(("zero-padded voxel read as wrapped", one_voxel((0, pad, pad), S[0, -1, 0, 0])))
    # 3. the last channel of a partial K-block read from the (zero) padding at one voxel
    if K % (32 if c.dtype == W.BF else 16):
        value = torch.zeros(K, dtype=torch.float64)
        value[K - 1] = -S[0, 0, 0, min(1, S.shape[3] - 1), K - 1]
        out.append(("channel of a partial K-block read from the padding", one_voxel((pad, pad, pad + min(1, S.shape[3] - 1)), value)))
    return out


def _b_setups():
    """(id, case, fp32 build): bf16 storage has one build, fp32 storage the split default and the exact one."""
    out = []
    for name in W.B_CASES:
        c = W.BY_NAME[name]
        out += [(name, c, False)] if c.dtype == W.BF else [(name + "_split", c, False), (name + "_exact", c, True)]
    return out


B_SETUPS = _b_setups()


@pytest.mark.parametrize("setup", B_SETUPS, ids=[s[0] for s in B_SETUPS])
def test_bound_admits_fp32_and_rejects_faults(setup):
    name, c, fp32_exact = setup
    info = W.plan_of(c)[1]
    bf16 = c.dtype == W.BF
    L, eps = W.depth(c, info, fp32_exact), R.eps_op(bf16, fp32_exact)
    epsm = R.eps_merge(W.family_of(info), W.cls_kind_of(info), bf16)
    xin, w = W.real_operands(c, 7)
    bias, nbias, res = W.epilogue_operands(c, 8, real=True)
    plain, abs_conv = W.ref(c, xin, w)
    ref, abs_sum = R.add_epilogue(plain, abs_conv, bias, nbias, res)
    bnd = R.bound(ref, abs_sum, abs_conv, L, eps, epsm, W.out_dtype(c) == W.BF)
    # 1. inside: the kernel's summation order in torch fp32, stored in the output type
    emu = emulate(c, info, xin, w, bias, nbias, res)
    err = (_store(emu, c) - ref).abs()
    print(f"{name}: fp32 emulation: max err / bound = {(err / bnd).max().item():.3f} (L = {L})")
    assert (err <= bnd).all(), f"{name}: the fp32 emulation lies outside the derived bound: {(err / bnd).max().item():.3f}"
    # 2. outside: the same emulation with one fault each
    for what, delta in _faults(c, info, xin, w):
        assert delta.abs().max().item() > 0, f"{name}: the emulated fault '{what}' changes nothing"
        err = (_store(emu + delta.float(), c) - ref).abs()
        print(f"{name}: {what}: max err / bound = {(err / bnd).max().item():.1f}")
        assert (err > bnd).any(), f"{name}: the bound (L = {L}) does not notice '{what}': {(err / bnd).max().item():.3f}"


def test_every_fault_is_emulated_on_some_case():
    names = set()
    for _, c, _ in B_SETUPS:
        xin, w = W.real_operands(c, 7)
        names |= {what for what, _ in _faults(c, W.plan_of(c)[1], xin, w)}
    assert names == {"dropped tap on a tile face", "zero-padded voxel read as wrapped",
                     "channel of a partial K-block read from the padding", "wrong merged tap"}
