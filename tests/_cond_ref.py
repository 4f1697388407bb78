"""References, bounds and the fp32 emulation of the K6 parity tests (csrc/cond.hip; cases in tests/_cond_cases.py).

  ref64    plain float64 restatement of the operation: sinusoid, two Linear + exact-erf GELU layers, projection, and its gradients
           written out by hand (tests/test_cond_cpu.py holds it against autograd of the oracle's own functions).
  ref_int  check A's reference: int64 arithmetic with ReLU (slope 1/2 at 0), never calling erf; asserts the four conditions of check A.
  bounds   check B's per-element running-error bound, counted from the code per case (see test_cond_kernels_gpu.py for the derivation).
  emulate  fp32 emulation of the kernels' order of operations in plain torch (per-lane fma chains, butterfly, slabs, folds, flat
           `saved` / `scratch`), with the faults of tests/test_cond_cpu.py as options.

All of them return one dict with the same keys: "table", "dbias", and per mlp k "k.emb", "k.h1", "k.h2", "k.c" (the four parts of
`saved`), "k.dh1", "k.dh2" (the rows of `scratch`), "k.dw1", "k.db1", "k.dw2", "k.db2", "k.dwproj", "k.din" (dL/dt [rows] for the
sinusoidal conditioning, dL/dv [rows, in_dim] for a vector)."""
import math

import torch

import _cond_cases as W

U = 2.0 ** -24
TINY = 2.0 ** -126
GELU_LIP = 1.12891          # sup |gelu'|  (at x = sqrt 2)
DGELU_LIP = 0.79789         # sup |gelu''| = 2 phi(0)
RSQRT2 = 0.7071067811865476
RSQRT2PI = 0.3989422804014327


def gamma(n):
    return n * U / (1.0 - n * U)


def freqs64(half):
    return torch.exp(-W.LN_1E4 * torch.arange(half, dtype=torch.float64) / half)


def embed64(t, in_dim):
    arg = 1000.0 * t.double()[:, None] * freqs64(in_dim // 2)[None, :]
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * RSQRT2))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x * RSQRT2)) + x * RSQRT2PI * torch.exp(-0.5 * x * x)


# ---- float64 reference ----------------------------------------------------------------------------------------------------------------
def ref64(ops, embs=None):
    """embs: per mlp None or the embedding to start from (check B gives the device's saved embedding, so that the error of the fp32
    sinusoid argument never enters the table or the gradients)."""
    dt = ops["dtable"].double()
    out = {"table": torch.zeros(ops["rows"], ops["width"], dtype=torch.float64), "dbias": dt.sum(0)}
    for k, m in enumerate(ops["mlps"]):
        w1, b1, w2, b2, wp = (m[n].double() for n in ("w1", "b1", "w2", "b2", "wproj"))
        if embs is not None and embs[k] is not None:
            x = embs[k].double()
        else:
            x = embed64(m["input"], m["in_dim"]) if m["sinusoid"] else m["input"].double()
        h1 = x @ w1.T + b1
        a1 = gelu64(h1)
        h2 = a1 @ w2.T + b2
        c = gelu64(h2)
        out["table"] += c @ wp.T
        dh2 = (dt @ wp) * dgelu64(h2)
        dh1 = (dh2 @ w2) * dgelu64(h1)
        g = dh1 @ w1
        if m["sinusoid"]:
            half = m["in_dim"] // 2
            F = 1000.0 * freqs64(half)
            g = (g[:, :half] * F * x[:, half:] - g[:, half:] * F * x[:, :half]).sum(1)
        out.update({f"{k}.emb": x, f"{k}.h1": h1, f"{k}.h2": h2, f"{k}.c": c, f"{k}.dh1": dh1, f"{k}.dh2": dh2,
                    f"{k}.dw1": dh1.T @ x, f"{k}.db1": dh1.sum(0), f"{k}.dw2": dh2.T @ a1, f"{k}.db2": dh2.sum(0),
                    f"{k}.dwproj": dt.T @ c, f"{k}.din": g})
    return out


# ---- check A: int64 reference with ReLU ---------------------------------------------------------------------------------------------
EXACT_LIMIT = 2 ** 22
BACKWARD = ("dh1", "dh2", "dw1", "db1", "dw2", "db2", "dwproj", "dbias", "din")


def _i(x):
    r = x.double().round().long()
    assert torch.equal(r.double(), x.double()), "check A: an operand is no integer"
    return r


def ref_int(ops, strict=True):
    """Check A's reference in int64.  gelu(x) = max(x, 0), gelu'(x) = 1, 1/2, 0 for x > 0, = 0, < 0: the backward carries 2 dh2 and
    4 dh1 as integers.  Returns (out, info): out as ref64 (float64, exact), minus the sinusoidal "k.din" (check B's);
    info = the largest sum of magnitudes, whether every column of every weight matrix carries a nonzero, the sign counts of h1 and h2,
    and the fourth condition's parts (below).  strict: assert the four conditions (otherwise only report them)."""
    dt = _i(ops["dtable"])
    big = 0
    cover = True
    signs = {"h1": [0, 0, 0], "h2": [0, 0, 0]}
    half_used = {"h1": False, "h2": False}
    layers_differ = False

    def mm(a, b):
        nonlocal big
        big = max(big, int((a.abs() @ b.abs()).max()))
        return a @ b

    out = {"dbias": dt.sum(0).double()}
    big = max(big, int(dt.abs().sum(0).max()))
    table = torch.zeros(ops["rows"], ops["width"], dtype=torch.int64)
    tabs = torch.zeros_like(table)
    for k, m in enumerate(ops["mlps"]):
        w1, b1, w2, b2, wp = (_i(m[n]) for n in ("w1", "b1", "w2", "b2", "wproj"))
        assert all(int(x.abs().max()) % 16 == 0 and torch.equal(x % 16, torch.zeros_like(x)) for x in (w1, b1, b2)), "w1, b1, b2: multiples of 16"
        cover = cover and all(bool((x != 0).any(0).all()) for x in (w1, w2, wp))
        if m["sinusoid"]:
            assert bool((m["input"] == 0).all()), "check A takes the sinusoidal conditioning at t = 0"
            half = m["in_dim"] // 2
            x = torch.cat([torch.zeros(ops["rows"], half, dtype=torch.int64), torch.ones(ops["rows"], half, dtype=torch.int64)], 1)
        else:
            x = _i(m["input"])
        h1 = mm(x, w1.T) + b1
        a1 = h1.clamp(min=0)
        h2 = mm(a1, w2.T) + b2
        c = h2.clamp(min=0)
        big = max(big, int(h1.abs().max()) + 32, int(h2.abs().max()) + 32)
        table += mm(c, wp.T)
        tabs += c.abs() @ wp.abs().T
        for name, h in (("h1", h1), ("h2", h2)):
            for j, cnt in enumerate(((h > 0).sum(), (h == 0).sum(), (h < 0).sum())):
                signs[name][j] += int(cnt)
        s2, s1 = 1 + torch.sign(h2), 1 + torch.sign(h1)                  # twice the slope
        dc = mm(dt, wp)
        d2 = dc * s2                                                     # 2 dh2
        da1 = mm(d2, w2)
        d1 = da1 * s1                                                    # 4 dh1
        half_used["h2"] = half_used["h2"] or bool(((h2 == 0) & (dc != 0)).any())
        half_used["h1"] = half_used["h1"] or bool(((h1 == 0) & (da1 != 0)).any())
        layers_differ = layers_differ or bool(((s1 != s2) & (dc != 0)).any())
        out.update({f"{k}.emb": x.double(), f"{k}.h1": h1.double(), f"{k}.h2": h2.double(), f"{k}.c": c.double(),
                    f"{k}.dh2": d2.double() / 2, f"{k}.dh1": d1.double() / 4,
                    f"{k}.dw1": mm(d1.T, x).double() / 4, f"{k}.db1": d1.sum(0).double() / 4,
                    f"{k}.dw2": mm(d2.T, a1).double() / 2, f"{k}.db2": d2.sum(0).double() / 2,
                    f"{k}.dwproj": mm(dt.T, c).double()})
        big = max(big, int(d1.abs().sum(0).max()), int(d2.abs().sum(0).max()))
        if not m["sinusoid"]:
            out[f"{k}.din"] = mm(d1, w1).double() / 4
    out["table"] = table.double()
    big = max(big, int(tabs.max()))
    # the fourth condition: the backward half is no comparison of 0 with 0.  Every backward tensor holds a nonzero; in each layer an
    # element with h == 0 meets a nonzero upstream gradient (the slope 1/2 is used); somewhere gelu'(h1) != gelu'(h2) under a nonzero
    # gradient (the two layers' slopes cannot be exchanged unseen)
    dead = [key for key, val in out.items() if key.split(".")[-1] in BACKWARD and not bool((val != 0).any())]
    info = dict(big=big, cover=cover, signs=signs, dead=dead, half_used=half_used, layers_differ=layers_differ)
    if strict:
        assert not dead, f"check A: backward tensors that are all 0: {dead}"
        assert all(half_used.values()), f"check A: no element with h == 0 carries a nonzero upstream gradient: {half_used}"
        assert layers_differ, "check A: gelu'(h1) == gelu'(h2) wherever the gradient is nonzero"
        # `big` counts 2 dh2 and 4 dh1 as the integers they are carried as: below 2^22 every fp32 sum of quarter-integers is exact
        assert big < EXACT_LIMIT, f"check A: a sum of magnitudes reaches {big} >= 2^22"
        assert cover, "check A: a column of a weight matrix holds no nonzero"
        assert all(min(s) > 0 for s in signs.values()), f"check A: h1 / h2 do not show all of > 0, == 0, < 0: {signs}"
    return out, info


def accept_a(ops):
    _, info = ref_int(ops, strict=False)
    return (info["big"] < EXACT_LIMIT and info["cover"] and all(min(s) > 0 for s in info["signs"].values())
            and not info["dead"] and all(info["half_used"].values()) and info["layers_differ"])


# ---- check B: the bound ---------------------------------------------------------------------------------------------------------------
def erf_terms(x):
    """Error of the device's 0.5 (1 + erff(x / sqrt 2)) at x, u already in: erff itself (K_ERF u |erf|), the rounded constant and the
    rounded product in its argument (2 u |z| erf'(z)), the addition 1 + erf."""
    z = x * RSQRT2
    e = torch.erf(z)
    return 0.5 * U * (W.K_ERF * e.abs() + 2.0 * z.abs() * (2.0 / math.sqrt(math.pi)) * torch.exp(-z * z) + (1.0 + e))


def gelu_err(h):
    """E_gelu(h): gelu_f(h) = (0.5 h) * (1 + erff(h c)): the terms of erf_terms times |h|, then the last product."""
    return h.abs() * erf_terms(h) + U * gelu64(h).abs() + TINY


def dgelu_err(h):
    """E_dgelu(h): the erf half as above; h * 0.3989.. * __expf(-0.5 h h): the exponential after _gn_bounds.silu_eval_err's model
    (relative 2 u (y + 2), y = h^2 / 2) plus its argument's one rounding (u y), the rounded constant and the two products (3 u); the
    last addition."""
    y = 0.5 * h * h
    return erf_terms(h) + (h.abs() * RSQRT2PI * torch.exp(-y)) * U * (3.0 * y + 7.0) + U * dgelu64(h).abs() + TINY


def dot_count(length, tpo, bias):
    """roundings one output of dot_row passes: the busiest lane's fmas, the butterfly, the bias addition"""
    return W.chain(length, tpo) + int(math.log2(tpo)) + (1 if bias else 0)


def embed_bound(t, in_dim):
    """|saved embedding - float64 sin / cos(1000 t f_i)|: the relative error of the device's f (K_FREQ u: the rounded quotient and
    product in expf's argument, about 2 * 9.21 u, and expf), the two products of 1000 * t * f (2 u), all times |arg| <= 1000, then
    sinf / cosf (K_SINCOS u |result|)."""
    half = in_dim // 2
    arg = (1000.0 * t.double()[:, None] * freqs64(half)[None, :]).abs()
    darg = arg * U * (W.K_FREQ + 2.0)
    e = embed64(t, in_dim)
    return torch.cat([darg, darg], 1) + W.K_SINCOS * U * e.abs() + TINY


def bounds(ops, R):
    """Per-element bound of |device - R| for R = ref64(ops, embs = the device's saved embeddings), same keys as R."""
    rows, width = ops["rows"], ops["width"]
    dt = ops["dtable"].double().abs()
    nslab = W.cdiv(width, W.BSLAB)
    n = len(ops["mlps"])
    E = {"dbias": gamma(rows) * dt.sum(0) + TINY}
    tab_abs = torch.zeros(rows, width, dtype=torch.float64)
    tab_err = torch.zeros(rows, width, dtype=torch.float64)
    for k, m in enumerate(ops["mlps"]):
        w1, b1, w2, b2, wp = (m[name].double().abs() for name in ("w1", "b1", "w2", "b2", "wproj"))
        in_dim, dim = m["in_dim"], m["dim"]
        tpo = W.tpo_for(dim)
        x, h1, h2, c, dh1, dh2 = (R[f"{k}.{name}"] for name in ("emb", "h1", "h2", "c", "dh1", "dh2"))
        a1 = gelu64(h1).abs()
        # forward
        e_h1 = gamma(dot_count(in_dim, tpo, True)) * (b1 + x.abs() @ w1.T) + TINY
        e_a1 = GELU_LIP * e_h1 + gelu_err(h1)
        e_h2 = gamma(dot_count(dim, tpo, True)) * (b2 + a1 @ w2.T) + e_a1 @ w2.T + TINY
        e_c = GELU_LIP * e_h2 + gelu_err(h2)
        tab_abs += c.abs() @ wp.T
        tab_err += gamma(dot_count(dim, 4, False)) * (c.abs() @ wp.T) + e_c @ wp.T
        # backward: slab partials (lane chain, LDS fold over nws), fold over the slabs (lane chain, LDS fold), one product with gelu'
        n_dc = W.cdiv(min(W.BSLAB, width), tpo) + tpo + W.cdiv(nslab, tpo) + tpo
        dc = ops["dtable"].double() @ m["wproj"].double()
        dc_abs = dt @ wp
        e_dc = gamma(n_dc) * dc_abs + TINY
        e_dh2 = e_dc * dgelu64(h2).abs() + (dc.abs() + e_dc) * (DGELU_LIP * e_h2 + dgelu_err(h2)) + U * dh2.abs() + TINY
        da1 = dh2 @ m["w2"].double()
        e_da1 = gamma(W.cdiv(dim, tpo) + tpo) * (dh2.abs() @ w2) + e_dh2 @ w2 + TINY
        e_dh1 = e_da1 * dgelu64(h1).abs() + (da1.abs() + e_da1) * (DGELU_LIP * e_h1 + dgelu_err(h1)) + U * dh1.abs() + TINY
        g_r = gamma(rows)
        E.update({f"{k}.h1": e_h1, f"{k}.h2": e_h2, f"{k}.c": e_c, f"{k}.dh1": e_dh1, f"{k}.dh2": e_dh2,
                  f"{k}.dw1": g_r * (dh1.abs().T @ x.abs()) + e_dh1.T @ x.abs() + TINY,
                  f"{k}.db1": g_r * dh1.abs().sum(0) + e_dh1.sum(0),
                  f"{k}.dw2": g_r * (dh2.abs().T @ a1) + e_dh2.T @ a1 + (dh2.abs() + e_dh2).T @ e_a1 + TINY,
                  f"{k}.db2": g_r * dh2.abs().sum(0) + e_dh2.sum(0),
                  f"{k}.dwproj": g_r * (dt.T @ c.abs()) + dt.T @ e_c + TINY})
        # K6i: the dim-long chain; for dL/dt the factor 1000 f_i (relative K_FREQ u, one more product for the 1000), two products, and
        # the 8-level LDS tree over all 256 threads
        g_abs = dh1.abs() @ w1
        e_g = gamma(dim) * g_abs + e_dh1 @ w1 + TINY
        if m["sinusoid"]:
            half = in_dim // 2
            F = 1000.0 * freqs64(half)
            sw = torch.cat([x[:, half:], x[:, :half]], 1).abs()                    # the saved value each g_i meets
            FF = torch.cat([F, F])
            g = dh1 @ m["w1"].double()
            terms = g.abs() * FF * sw
            E[f"{k}.din"] = (e_g * FF * sw + terms * U * (W.K_FREQ + 3.0)).sum(1) + gamma(8) * terms.sum(1) + TINY
        else:
            E[f"{k}.din"] = e_g
    E["table"] = tab_err + gamma(n - 1) * tab_abs + TINY if n > 1 else tab_err + TINY
    return E


def ratios(got, R, E, keys=None):
    """{key: max over the elements of |got - R| / E}; a NaN anywhere gives inf."""
    out = {}
    for key in (keys or [key for key in R if key in E]):
        r = (got[key].double() - R[key]).abs() / E[key]
        out[key] = float("inf") if bool(torch.isnan(r).any()) else r.max().item()
    return out


def worst_by_tensor(rat):
    """{tensor name without the mlp index: worst ratio}"""
    out = {}
    for key, r in rat.items():
        name = key.split(".")[-1]
        out[name] = max(out.get(name, 0.0), r)
    return out


# ---- fp32 emulation of the kernels' order -----------------------------------------------------------------------------------------------
FAULTS = ("last_dropped", "tail_dropped", "fslab_off_by_one", "bslab_off_by_one", "second_fold_dropped", "dgelu_at_h1", "no_half_at_0",
          "tanh_gelu", "saved_offset_mlp0", "dtable_stride_width", "sincos_exchanged", "freq_half_minus_1")


def fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 is exact in float64, the sum rounds to 53 bits and then to 24 (a double rounding
    that differs from the fused result only on ties of the second rounding, far inside the bound)."""
    return (a.double() * b.double() + c.double()).float()


def _erf32(x):
    return torch.erf(x * torch.tensor(RSQRT2, dtype=torch.float32))


def gelu32(x, fault=None):
    if fault == "tanh_gelu":
        return torch.nn.functional.gelu(x, approximate="tanh")
    return (0.5 * x) * (1.0 + _erf32(x))


def dgelu32(x, fault=None):
    if fault == "tanh_gelu":
        xd = x.double().requires_grad_(True)
        torch.nn.functional.gelu(xd, approximate="tanh").sum().backward()
        return xd.grad.float()
    d = 0.5 * (1.0 + _erf32(x)) + (x * torch.tensor(RSQRT2PI, dtype=torch.float32)) * torch.exp((-0.5 * x) * x)
    if fault == "no_half_at_0":
        d = torch.where(x == 0, torch.zeros_like(d), d)
    return d


def _lane_indices(length, tpo, fault):
    nq = W.quads(length)
    end = 4 * (length // 4) if fault == "tail_dropped" else length
    lanes = []
    for s in range(tpo):
        idx = [4 * q + e for q in range(s, nq, tpo) for e in range(4)] + list(range(4 * nq + s, end, tpo))
        if fault == "last_dropped":
            idx = [i for i in idx if i != length - 1]
        lanes.append(idx)
    return lanes


def dot_row32(w, x, tpo, fault=None):
    """[R, len] x [O, len] -> [R, O] in the order of dot_row: per lane the quads of its stride, then its share of the tail, then the
    xor butterfly over the lanes."""
    lanes = _lane_indices(w.shape[1], tpo, fault)
    acc = []
    for idx in lanes:
        a = torch.zeros(x.shape[0], w.shape[0])
        for i in idx:
            a = fma(w[None, :, i], x[:, None, i], a)
        acc.append(a)
    o = 1
    while o < tpo:
        acc = [acc[s] + acc[s ^ o] for s in range(tpo)]
        o <<= 1
    return acc[0]


def _strided_fold(term, count, nws, limit=None):
    """sum over j < count of term(j) the way the backward kernels do: lane ws takes j = ws, ws + nws, ... in order (term returns the
    updated accumulator), then lane 0 adds the lanes in order.  limit: only the first `limit` j of every lane (a dropped later pass)."""
    lanes = []
    for ws in range(nws):
        s = None
        js = list(range(ws, count, nws))
        for j in (js if limit is None else js[:limit]):
            s = term(j, s)
        lanes.append(s)
    tot = None
    for s in lanes:
        if s is not None:
            tot = s if tot is None else tot + s
    return tot


def embed32(t, in_dim, fault=None):
    half = in_dim // 2
    i = torch.arange(half, dtype=torch.float32)
    den = torch.tensor(float(half - 1 if fault == "freq_half_minus_1" else half), dtype=torch.float32)
    f = torch.exp(torch.tensor(-W.LN_1E4, dtype=torch.float32) * i / den)
    arg = (torch.tensor(1000.0) * t.float())[:, None] * f[None, :]
    s, c = torch.sin(arg), torch.cos(arg)
    return torch.cat([c, s] if fault == "sincos_exchanged" else [s, c], 1)


def emulate(ops, fault=None, stride_pad=5):
    """The four kernels in fp32, in their order of operations, through flat `saved` and `scratch` buffers laid out as the code lays them
    out; dtable is a column block of a [rows, width + stride_pad] NaN-filled matrix."""
    assert fault is None or fault in FAULTS, fault
    rows, width, ms = ops["rows"], ops["width"], ops["mlps"]
    n = len(ms)
    nslab = W.cdiv(width, W.BSLAB)
    svs = [m["in_dim"] + 3 * m["dim"] for m in ms]

    def saved_base(k):
        return sum(rows * (svs[0] if fault == "saved_offset_mlp0" else svs[q]) for q in range(k))

    saved = torch.full((max(sum(rows * s for s in svs), saved_base(n - 1) + rows * svs[-1]),), float("nan"))

    def sv_view(k):
        return saved[saved_base(k):saved_base(k) + rows * svs[k]].view(rows, svs[k])

    f_elem = None if fault not in ("last_dropped", "tail_dropped") else fault
    # ---- forward
    table = torch.full((rows, width), float("nan"))
    cs = []
    for k, m in enumerate(ms):
        i_d, d = m["in_dim"], m["dim"]
        tpo = W.tpo_for(d)
        x = embed32(m["input"], i_d, fault) if m["sinusoid"] else m["input"].float()
        h1 = m["b1"][None, :] + dot_row32(m["w1"], x, tpo, f_elem)
        a1 = gelu32(h1, fault)
        h2 = m["b2"][None, :] + dot_row32(m["w2"], a1, tpo, f_elem)
        c = gelu32(h2, fault)
        cs.append(c)
        sv = sv_view(k)
        sv[:, :i_d], sv[:, i_d:i_d + d], sv[:, i_d + d:i_d + 2 * d], sv[:, i_d + 2 * d:] = x, h1, h2, c
    acc = torch.zeros(rows, width)
    for k, m in enumerate(ms):
        acc = acc + dot_row32(m["wproj"], cs[k], 4, f_elem)
    slab_cols = W.FSLAB - 1 if fault == "fslab_off_by_one" else W.FSLAB
    written = (torch.arange(width) % W.FSLAB) < slab_cols
    table[:, written] = acc[:, written]
    # ---- backward
    stride = width + stride_pad
    wide = torch.full((rows * stride + 2 * stride_pad,), float("nan"))
    base = 2
    for r in range(rows):
        wide[base + r * stride:base + r * stride + width] = ops["dtable"][r]
    rd = width if fault == "dtable_stride_width" else stride
    dt = torch.stack([wide[base + r * rd:base + r * rd + width] for r in range(rows)])
    out = {"table": table}
    dbias = torch.zeros(width)
    for r in range(rows):
        dbias = dbias + dt[r]
    out["dbias"] = dbias
    for k, m in enumerate(ms):
        i_d, d = m["in_dim"], m["dim"]
        nws = W.tpo_for(d)
        sv = sv_view(k)                                     # the backward reads what the forward saved, through the same offsets
        x, h1, h2, c = sv[:, :i_d], sv[:, i_d:i_d + d], sv[:, i_d + d:i_d + 2 * d], sv[:, i_d + 2 * d:]
        wp, w2, w1 = m["wproj"], m["w2"], m["w1"]
        parts = []
        for s in range(nslab):
            w0 = s * W.BSLAB
            wn = min(W.BSLAB, width - w0) - (1 if fault == "bslab_off_by_one" else 0)
            p = _strided_fold(lambda j, a: fma(dt[:, w0 + j, None], wp[None, w0 + j, :], torch.zeros(rows, d) if a is None else a), wn, nws)
            parts.append(torch.zeros(rows, d) if p is None else p)
        limit = W.FOLD_PER_PASS if fault == "second_fold_dropped" else None
        dc = _strided_fold(lambda j, a: parts[j] if a is None else a + parts[j], nslab, nws, limit)
        dh2 = dc * dgelu32(h1 if fault == "dgelu_at_h1" else h2, fault)
        da1 = _strided_fold(lambda j, a: fma(dh2[:, j, None], w2[None, j, :], torch.zeros(rows, d) if a is None else a), d, nws)
        dh1 = da1 * dgelu32(h1, fault)
        a1 = gelu32(h1, fault)
        dw1, dw2, dwp = torch.zeros(d, i_d), torch.zeros(d, d), torch.zeros(width, d)
        db1, db2 = torch.zeros(d), torch.zeros(d)
        for r in range(rows):
            dw1 = fma(dh1[r, :, None], x[r, None, :], dw1)
            dw2 = fma(dh2[r, :, None], a1[r, None, :], dw2)
            dwp = fma(dt[r, :, None], c[r, None, :], dwp)
            db1, db2 = db1 + dh1[r], db2 + dh2[r]
        g = torch.zeros(rows, i_d)
        for j in range(d):
            g = fma(dh1[:, j, None], w1[None, j, :], g)
        if m["sinusoid"]:
            half = i_d // 2
            i = torch.arange(half, dtype=torch.float32)
            f = torch.tensor(1000.0) * torch.exp(torch.tensor(-W.LN_1E4, dtype=torch.float32) * i / torch.tensor(float(half)))
            red = torch.zeros(rows, 256)
            red[:, :half] = (g[:, :half] * f) * x[:, half:]
            red[:, half:i_d] = (-g[:, half:] * f) * x[:, :half]
            wdt = 128
            while wdt > 0:
                red[:, :wdt] = red[:, :wdt] + red[:, wdt:2 * wdt]
                wdt >>= 1
            g = red[:, 0]
        # what a caller unpacks from `saved` with the layout the ABI states
        off = sum(rows * svs[q] for q in range(k))
        true = saved[off:off + rows * svs[k]].view(rows, svs[k])
        out.update({f"{k}.emb": true[:, :i_d].clone(), f"{k}.h1": true[:, i_d:i_d + d].clone(), f"{k}.h2": true[:, i_d + d:i_d + 2 * d].clone(),
                    f"{k}.c": true[:, i_d + 2 * d:].clone(), f"{k}.dh1": dh1, f"{k}.dh2": dh2, f"{k}.dw1": dw1, f"{k}.db1": db1,
                    f"{k}.dw2": dw2, f"{k}.db2": db2, f"{k}.dwproj": dwp, f"{k}.din": g})
    return out
