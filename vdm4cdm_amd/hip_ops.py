"""Typed wrappers over the C-ABI: torch tensors in, kernels enqueued on torch's current HIP stream.

torch is used here only for device memory and streams (``Tensor.data_ptr()``,
``torch.cuda.current_stream()``); no torch compute op runs on activations in this module.
Activations are NDHWC tensors ``[N, D, H, W, C]`` (fp32 or bf16).
"""
import ctypes as C

import torch

from . import _experiment, _lib
from ._lib import CondMlp, ConvDesc, GnFold, PACK_DGRAD, PACK_FWD, VDM_BF16, VDM_F32, check

GN_EPS = 1e-5
# timing ablations (tools/ablate_step.sh): kernels named here are NOT launched (wrong results - only bench.py timing runs set this)
ABLATE = set(_experiment.get("ablate"))
FUSED_TAIL = bool(_experiment.get("fused_tail"))      # gn_tail_ok (fused_tail=0: separate apply pass and weight gradient, for A/B timing)


class KernelProfiler:
    """Optional per-launch HIP-event timing (bench.py): events are recorded on the launch stream around each
    C-ABI call; `summary()` aggregates per kernel key after a synchronize."""

    def __init__(self, tags=None):
        self.records = []          # (key, start, end, flops, bytes)
        self.tags = tags           # None: every launch; else only launches whose tag is in this set (event records cost time too)
        self.main_stream = None    # launches on any other stream are marked "side" (weight gradients, skip convs: off the critical path)

    def begin(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, start, key, flops=0.0, nbytes=0.0, exec_flops=None):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        if self.main_stream is None:
            self.main_stream = torch.cuda.default_stream().cuda_stream
        side = torch.cuda.current_stream().cuda_stream != self.main_stream
        self.records.append((key, start, e, flops, nbytes, flops if exec_flops is None else exec_flops, side))

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for key, s, e, fl, nb, xf, side in self.records:
            a = agg.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "exec_flops": 0.0, "side_launches": 0})
            a["launches"] += 1
            a["side_launches"] += 1 if side else 0
            a["ms"] += s.elapsed_time(e)
            a["flops"] += fl
            a["bytes"] += nb
            a["exec_flops"] += xf
        return agg


PROFILER = None        # set to a KernelProfiler by bench.py
# Device step counter (int32 tensor) mixed into every RNG seed inside the kernels (dropout masks, noise fields, time grid); set by
# vdm_model.GraphedTrainStep: a captured graph bakes the host seeds into its kernel arguments, the counter keeps the draws fresh.
SEED_STEP = None


def _pb(tag="other"):
    if PROFILER is None or (PROFILER.tags is not None and tag not in PROFILER.tags):
        return None
    return PROFILER.begin()


def _pe(ev, key, flops=0.0, nbytes=0.0, exec_flops=None):
    """flops: algorithmic (27 taps on the conv's own grid); exec_flops: what the kernel issues to the matrix cores (the
    per-parity-class kernels run 8 merged taps / 1-8 taps per class instead of 27)."""
    if ev is not None:
        PROFILER.end(ev, key, flops, nbytes, exec_flops)


def _nc_for(cout, dtype=None):
    return 1 if cout <= 16 else (2 if (cout <= 32 or dtype == torch.float32) else 4)


def _tname(dtype):
    return "float" if dtype == torch.float32 else "bf16_t"


def dt_id(dtype):
    if dtype == torch.float32:
        return VDM_F32
    if dtype == torch.bfloat16:
        return VDM_BF16
    raise ValueError(f"unsupported activation dtype {dtype}")


def epl(dtype):
    """elements per 16-byte piece"""
    return 4 if dtype == torch.float32 else 8


def cpad(c, dtype):
    e = epl(dtype)
    return (c + e - 1) // e * e


def _s():
    return torch.cuda.current_stream().cuda_stream


def _scratch(cache, key, numel, dtype, device, floor=0):
    """Per-(device, stream) scratch tensors are cached in module-level dicts - EXCEPT while the current stream is being captured into a
    hipGraph: an allocation made during capture comes out of that graph's private memory pool, the pool keeps the block for the replays
    whether or not the tensor object survives, and a module-level reference would pin memory of a pool whose graph is long gone (and
    hand it to later captures / eager launches on a stream that happens to reuse the handle).  Under capture: a fresh tensor, not cached."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(numel, floor), dtype=dtype, device=device)
    ws = cache.get(key)
    if ws is None or ws.numel() < numel:
        ws = cache[key] = torch.empty(max(numel, floor), dtype=dtype, device=device)
    return ws


# The side stream a launch is being issued on (set by unet_hip.SideStream.run around its body), else None.  Every tensor whose pointer
# goes to a kernel while it is set is recorded on that stream HERE - one choke point instead of a record_stream per call site: memory
# that was allocated on the main stream and is still referenced by a queued side-stream kernel (weight gradients run up to a whole
# backward pass behind the main stream) cannot be handed to a new owner by the caching allocator before that kernel has run.
SIDE_STREAM = None


def _p(t):
    if t is None:
        return None
    assert t.is_cuda, "HIP ops need device tensors"
    if SIDE_STREAM is not None:
        t.record_stream(SIDE_STREAM)
    return t.data_ptr()


def _contig(*ts):
    for t in ts:
        if t is not None:
            assert t.is_contiguous(), "HIP ops need contiguous tensors"


class Conv:
    """One convolution layer: descriptor factory + packed-weight buffers (fwd / dgrad order)."""

    _ws = {}          # (device, stream) -> wgrad workspace (uint8 tensor): launches on one stream are ordered, streams never share

    def __init__(self, cin, cout, ksize=3, stride=1, upsample=0, circular=False, out_f32=False):
        self.cin, self.cout, self.ksize, self.stride, self.upsample = cin, cout, ksize, stride, upsample
        self.circular, self.out_f32 = circular, out_f32
        self.wf = self.wd = None
        self._descs = {}

    def desc(self, n, od, oh, ow, dtype, stride=None):
        st = self.stride if stride is None else stride
        key = (n, od, oh, ow, dtype, st)
        d = self._descs.get(key)
        if d is None:
            d = ConvDesc(n=n, od=od, oh=oh, ow=ow, cin=self.cin, cout=self.cout, ksize=self.ksize, stride=st,
                         upsample=self.upsample, pad_mode=1 if self.circular else 0, dtype=dt_id(dtype),
                         out_f32=1 if (self.out_f32 and st == self.stride) else 0)
            self._descs[key] = d
        return d

    def pack(self, w_master, dtype, need_dgrad):
        """w_master: fp32 [taps, cout, cin] (a view into the flat parameter vector)."""
        L = _lib.lib()
        d = self.desc(1, 2, 2, 2, dtype)
        assert w_master.dtype == torch.float32 and w_master.is_contiguous()
        assert w_master.numel() == self.ksize ** 3 * self.cout * self.cin
        self.alloc_packed(w_master.device, dtype, need_dgrad)
        check(L.vdm_conv_pack_weights(d, PACK_FWD, _p(w_master), _p(self.wf), _s()), "vdm_conv_pack_weights(fwd)")
        if need_dgrad:
            check(L.vdm_conv_pack_weights(d, PACK_DGRAD, _p(w_master), _p(self.wd), _s()), "vdm_conv_pack_weights(dgrad)")

    def alloc_packed(self, device, dtype, need_dgrad):
        """Make sure the packed-weight buffers exist (pack / pack_many fill them)."""
        L = _lib.lib()
        d = self.desc(1, 2, 2, 2, dtype)
        if self.wf is None or self.wf.device != device or self._packed_dtype != dtype:
            self.wf = torch.empty(L.vdm_conv_packed_bytes(d, PACK_FWD), dtype=torch.uint8, device=device)
            self.wd = None
            self._packed_dtype = dtype
        if need_dgrad and self.wd is None:
            self.wd = torch.empty(L.vdm_conv_packed_bytes(d, PACK_DGRAD), dtype=torch.uint8, device=device)

    def _kernel_key(self, d, dgrad, dtype):
        """Profiler key of the kernel family that runs this conv in one direction (one vdm_conv_kernel_variant call; a rolling-z
        launch keeps the plain conv_fwd_kernel key)."""
        var = _lib.lib().vdm_conv_kernel_variant(d, dgrad)
        t, nc = _tname(dtype), _nc_for(self.cin if dgrad else self.cout, dtype)
        if var == 1:
            return f"conv_cls_kernel<{t},NC{nc},{'B' if dgrad and self.upsample else 'F'}>"
        if var == 2:
            return "conv_kpack_kernel"
        if var == 3:
            return f"conv_fwd_kernel<{t},k3,s1,NC2,split>"
        if var == 4:
            return f"conv_ksplit_kernel<{t},NC4>"
        return f"conv_fwd_kernel<{t},k{self.ksize},s{1 if dgrad else self.stride},NC{nc}>"

    def out_shape(self, x):
        n, d, h, w, _ = x.shape
        if self.stride == 2:
            return (n, d // 2, h // 2, w // 2, self.cout)
        if self.upsample:
            return (n, 2 * d, 2 * h, 2 * w, self.cout)
        return (n, d, h, w, self.cout)

    def fwd(self, x, bias=None, nbias=None, residual=None, out=None, gn=False):
        """out = conv(x) + bias + nbias[n] + residual.  nbias: fp32 [N, >=cout] view (row stride honoured)."""
        L = _lib.lib()
        _contig(x, bias, residual)
        assert x.shape[-1] == cpad(self.cin, x.dtype), f"conv input must have {cpad(self.cin, x.dtype)} channels, got {x.shape[-1]}"
        shp = self.out_shape(x)
        if out is None:
            out = torch.empty(shp, dtype=torch.float32 if self.out_f32 else x.dtype, device=x.device)
        assert tuple(out.shape) == shp and out.is_contiguous()
        nstride = 0
        if nbias is not None:
            assert nbias.dtype == torch.float32 and nbias.stride(1) == 1 and nbias.shape[0] == x.shape[0]
            nstride = nbias.stride(0)
        if residual is not None:
            assert residual.shape == out.shape and residual.dtype == x.dtype
        d = self.desc(shp[0], shp[1], shp[2], shp[3], x.dtype)
        part = None
        if gn:                    # GroupNorm statistics of `out`, reduced per tile by the epilogue; consumed by gn_stats(out, ...)
            tiles = L.vdm_conv_gn_tiles(d)
            if tiles > 0:
                part = torch.empty((shp[0], tiles, self.cout, 2), dtype=torch.float32, device=x.device)
        if "conv1" in ABLATE and self.ksize == 1:
            out.gn_partials = None
            return out
        ev = _pb("conv3" if self.ksize == 3 else "other")
        check(L.vdm_conv_fwd(d, _p(x), _p(self.wf), _p(bias), _p(nbias), nstride, _p(residual), _p(out), _p(part), _s()), "vdm_conv_fwd")
        out.gn_partials = part
        if ev is not None:
            nvox = shp[0] * shp[1] * shp[2] * shp[3]
            es = x.element_size()
            alg = 2.0 * nvox * self.ksize ** 3 * self.cin * self.cout
            _pe(ev, self._kernel_key(d, 0, x.dtype), alg,
                x.numel() * es + out.numel() * out.element_size() + (residual.numel() * es if residual is not None else 0),
                alg * (8.0 / 27.0) if (self.ksize == 3 and self.upsample) else None)          # 8 merged taps per parity class
        return out

    def dgrad(self, dout, residual=None, out=None):
        """Gradient w.r.t. the conv input (stride 2: twice the dout dims; up-sampling conv: half)."""
        L = _lib.lib()
        _contig(dout, residual)
        n, od, oh, ow, c = dout.shape
        assert c == cpad(self.cout, dout.dtype)
        if self.stride == 2:
            ishape = (n, 2 * od, 2 * oh, 2 * ow, self.cin)
        elif self.upsample:
            ishape = (n, od // 2, oh // 2, ow // 2, self.cin)
        else:
            ishape = (n, od, oh, ow, self.cin)
        if out is None:
            out = torch.empty(ishape, dtype=dout.dtype, device=dout.device)
        assert tuple(out.shape) == ishape and (residual is None or tuple(residual.shape) == ishape)
        d = self.desc(n, od, oh, ow, dout.dtype)
        if "conv1" in ABLATE and self.ksize == 1:
            return out
        ev = _pb("conv3" if self.ksize == 3 else "other")
        check(L.vdm_conv_dgrad(d, _p(dout), _p(self.wd), _p(residual), _p(out), _s()), "vdm_conv_dgrad")
        if ev is not None:
            nvox = n * od * oh * ow
            es = dout.element_size()
            alg = 2.0 * nvox * self.ksize ** 3 * self.cin * self.cout
            xf = None
            if self.ksize == 3 and self.upsample:
                xf = alg * (8.0 / 27.0)                       # 8 classes x 8 merged taps on the coarse grid (= 64/216 of 27 fine taps)
            elif self.ksize == 3 and self.stride == 2:
                xf = alg                                      # 27 taps in total over the 8 classes of the fine grid: nothing skipped
            _pe(ev, self._kernel_key(d, 1, dout.dtype), alg,
                dout.numel() * es + out.numel() * es + (residual.numel() * es if residual is not None else 0), xf)
        return out

    def gn_fold_ok(self, c1, c2, dtype):
        """Can dgrad_gn be used for a GroupNorm over concat(c1, c2) = this conv's input channels?  (a lane's 4*NC consecutive
        channels must not straddle the concat boundary; 3x3x3 stride-1 convs only)"""
        span = 4 * _nc_for(self.cin, dtype)
        return (self.ksize == 3 and self.stride == 1 and not self.upsample and c1 + c2 == self.cin and self.cin % span == 0
                and (c2 == 0 or c1 % span == 0) and self.cin % epl(dtype) == 0)

    def dgrad_gn(self, dout, x1, x2, groups, stats, gamma, beta, keep_mask=None, dropout_p=0.0, out=None):
        """Input gradient of a conv whose input was drop(silu(gn(concat(x1, x2)))), with the GroupNorm backward reduction folded
        into the epilogue.  Returns dyh = dL/dy * keep/(1-p) * silu'(yhat) with `.gnb_partials` ([N, tiles, cin, 2]: per-tile
        sums of dyh and dyh * x) for gn_bwd_finalize."""
        L = _lib.lib()
        _contig(dout, x1, x2, stats, gamma, beta, keep_mask)
        n, od, oh, ow, c = dout.shape
        assert c == cpad(self.cout, dout.dtype)
        c1, c2 = x1.shape[-1], (0 if x2 is None else x2.shape[-1])
        assert self.gn_fold_ok(c1, c2, dout.dtype), "dgrad_gn: unsupported channel split"
        assert tuple(x1.shape[:-1]) == (n, od, oh, ow) and x1.dtype == dout.dtype
        if out is None:
            out = torch.empty((n, od, oh, ow, self.cin), dtype=dout.dtype, device=dout.device)
        d = self.desc(n, od, oh, ow, dout.dtype)
        tiles = L.vdm_conv_dgrad_gn_tiles(d)
        part = torch.empty((n, tiles, self.cin, 2), dtype=torch.float32, device=dout.device)
        f = GnFold(x1=_p(x1), x2=_p(x2), c1=c1, c2=c2, groups=groups, stats=_p(stats), gamma=_p(gamma), beta=_p(beta), eps=GN_EPS,
                   inv_keep=1.0 / (1.0 - dropout_p) if keep_mask is not None else 1.0, keep_mask=_p(keep_mask), partials=_p(part))
        ev = _pb("conv3")
        check(L.vdm_conv_dgrad_gn(d, _p(dout), _p(self.wd), _p(out), C.byref(f), _s()), "vdm_conv_dgrad_gn")
        out.gnb_partials = part
        if ev is not None:
            es = dout.element_size()
            _pe(ev, self._kernel_key(d, 1, dout.dtype) + "+gnb", 2.0 * n * od * oh * ow * 27 * self.cin * self.cout,
                dout.numel() * es + 2 * out.numel() * es)
        return out

    def wgrad(self, x, dout, dw, dbias=None, accumulate=False):
        """dw (fp32 view [taps, cout, cin]) = sum_v dout[v] (x) x[v + tap];  dbias (optional, ksize 3): sum_v dout[v]."""
        L = _lib.lib()
        _contig(x, dout, dw)
        n, od, oh, ow, c = dout.shape
        assert c == cpad(self.cout, dout.dtype) and x.shape[-1] == cpad(self.cin, x.dtype)
        d = self.desc(n, od, oh, ow, x.dtype)
        need = L.vdm_conv_wgrad_workspace_bytes(d)
        ws = _scratch(Conv._ws, (x.device, _s()), need, torch.uint8, x.device, floor=32 << 20)
        if "wgrad" in ABLATE or ("wgrad1" in ABLATE and self.ksize == 1):
            return dw
        ev = _pb("wgrad" if self.ksize == 3 else "other")
        check(L.vdm_conv_wgrad(d, _p(x), _p(dout), _p(dw), _p(dbias), 1 if accumulate else 0, _p(ws), ws.numel(), _s()), "vdm_conv_wgrad")
        if ev is not None:
            es = x.element_size()
            alg = 2.0 * n * od * oh * ow * self.ksize ** 3 * self.cin * self.cout
            _pe(ev, f"conv_wgrad_kernel<{_tname(x.dtype)},k{self.ksize},s{self.stride},u{self.upsample}>+reduce",
                alg, x.numel() * es + dout.numel() * es, alg * (8.0 / 27.0) if (self.ksize == 3 and self.upsample) else None)
        return dw


def _nv(x):
    n = x.shape[0]
    return n, x.numel() // (n * x.shape[-1])


_gn_ws = {}


def gn_stats(x1, x2, groups, out=None, chsum=False):
    """stats[n][g] = (sum, sum of squares) of concat(x1, x2).  chsum=True (sources produced by Conv.fwd(gn=True) only): also the
    per-channel sums, attached as `out.chsum` ([N, C] fp32)."""
    L = _lib.lib()
    _contig(x1, x2)
    n, v = _nv(x1)
    if out is None:
        out = torch.empty((n, groups, 2), dtype=torch.float32, device=x1.device)
    ws = _scratch(_gn_ws, (x1.device, _s()), _lib.GN_STATS_WS_BYTES // 4, torch.float32, x1.device)
    c2 = 0 if x2 is None else x2.shape[-1]
    p1 = getattr(x1, "gn_partials", None)       # set by Conv.fwd(..., gn=True): that source needs no pass over the tensor
    p2 = getattr(x2, "gn_partials", None) if x2 is not None else None
    cs = None
    if chsum and p1 is not None and (x2 is None or p2 is not None):
        cs = torch.empty((n, x1.shape[-1] + c2), dtype=torch.float32, device=x1.device)
    ev = _pb()
    check(L.vdm_gn_stats(_p(x1), x1.shape[-1], _p(x2), c2, n, v, groups, dt_id(x1.dtype), _p(out), _p(ws),
                         _p(p1), 0 if p1 is None else p1.shape[1], _p(p2), 0 if p2 is None else p2.shape[1], _p(cs), _s()), "vdm_gn_stats")
    out.chsum = cs
    _pe(ev, "gn_stats", 0.0, (x1.numel() * x1.element_size() if p1 is None else 0)
        + (x2.numel() * x2.element_size() if (x2 is not None and p2 is None) else 0))
    return out


def gn_silu_fwd(x1, x2, groups, stats, gamma, beta, dropout_p=0.0, seed=0, out=None, want_mask=False, linear=False):
    """want_mask (with dropout_p > 0): the dropout keep bits are also written, one byte per 16-byte piece, attached as
    `out.keep_mask` (consumed by Conv.dgrad_gn)."""
    L = _lib.lib()
    _contig(x1, x2, gamma, beta, stats)
    n, v = _nv(x1)
    c1 = x1.shape[-1]
    c2 = 0 if x2 is None else x2.shape[-1]
    if out is None:
        out = torch.empty(x1.shape[:-1] + (c1 + c2,), dtype=x1.dtype, device=x1.device)
    mask = None
    if want_mask and dropout_p > 0.0:
        mask = torch.empty((n, v, (c1 + c2) // epl(x1.dtype)), dtype=torch.uint8, device=x1.device)
    if "gn_fwd" in ABLATE:
        out.keep_mask = mask
        return out
    ev = _pb()
    check(L.vdm_gn_silu_fwd(_p(x1), c1, _p(x2), c2, n, v, groups, dt_id(x1.dtype), _p(stats), _p(gamma), _p(beta), GN_EPS,
                            float(dropout_p), int(seed), _p(out), _p(mask), int(bool(linear)), _p(SEED_STEP), _s()), "vdm_gn_silu_fwd")
    out.keep_mask = mask
    _pe(ev, "gn_silu_fwd", 0.0, 2.0 * out.numel() * out.element_size())
    return out


def gn_skip_supported(c1, c2, cout, dtype):
    """(forward, backward): whether the 1x1x1 skip conv (c1 + c2 -> cout) can ride along with norm1's GroupNorm passes
    (csrc/gn_skip.hip: bf16 storage, narrow layers)."""
    if dtype != torch.bfloat16:
        return False, False
    m = _lib.lib().vdm_gn_skip_supported(int(c1), int(c2), int(cout), dt_id(dtype))
    return bool(m & 1), bool(m & 2)


def gn_silu_skip_fwd(x1, x2, groups, stats, gamma, beta, w1, w2, bias):
    """(silu(gn(concat(x1, x2))), w1 x1 + w2 x2 + bias) in one pass over the block input: norm1 + the 1x1x1 skip conv of a ResNetBlock.
    w1 / w2: fp32 master weights [cout, c1(, 1, 1, 1)] / [cout, c2(, 1, 1, 1)] (w2 None without a second source)."""
    L = _lib.lib()
    _contig(x1, x2, gamma, beta, stats, w1, w2, bias)
    n, v = _nv(x1)
    c1 = x1.shape[-1]
    c2 = 0 if x2 is None else x2.shape[-1]
    cout = w1.shape[0]
    y = torch.empty(x1.shape[:-1] + (c1 + c2,), dtype=x1.dtype, device=x1.device)
    sk = torch.empty(x1.shape[:-1] + (cout,), dtype=x1.dtype, device=x1.device)
    y.keep_mask = None
    if "gn_fwd" in ABLATE:
        return y, sk
    ev = _pb()
    check(L.vdm_gn_silu_skip_fwd(_p(x1), c1, _p(x2), c2, n, v, groups, dt_id(x1.dtype), _p(stats), _p(gamma), _p(beta), GN_EPS,
                                 _p(w1), _p(w2), _p(bias), cout, _p(y), _p(sk), _s()), "vdm_gn_silu_skip_fwd")
    _pe(ev, "gn_silu_fwd", 2.0 * n * v * (c1 + c2) * cout, (2.0 * y.numel() + sk.numel()) * y.element_size())
    return y, sk


_skip_ws = {}


def gn_silu_bwd(x1, x2, groups, stats, gamma, beta, dy, dgamma, dbeta, add1=None, add2=None, colsum=None,
                dropout_p=0.0, seed=0, dx1=None, dx2=None, linear=False):
    """GroupNorm(+SiLU+dropout) backward for a gradient `dy` that did NOT come out of Conv.dgrad_gn: dyh = dy * keep * silu'(yhat) as
    its own pass (vdm_gn_dyh), its per-sample channel totals (vdm_channel_dot_sums), then the fixed-order finalize + apply kernels of
    the folded path (gn_bwd_fused) - bit-reproducible, no float atomics.  Returns (dx1, dx2); writes dgamma / dbeta and, if given,
    colsum[n, c] = sum_v dx (bias / conditioning-table gradients)."""
    L = _lib.lib()
    _contig(x1, x2, dy, add1, add2, gamma, beta, dgamma, dbeta, stats)
    n, v = _nv(x1)
    c1 = x1.shape[-1]
    c2 = 0 if x2 is None else x2.shape[-1]
    ev = _pb()
    dyh = dy if (dx1 is not None and dx1.data_ptr() == dy.data_ptr()) else torch.empty_like(dy)      # in place when the caller gave dy away
    check(L.vdm_gn_dyh(_p(x1), c1, _p(x2), c2, n, v, groups, dt_id(x1.dtype), _p(stats), _p(gamma), _p(beta), GN_EPS, float(dropout_p),
                       int(seed), _p(dy), _p(dyh), int(bool(linear)), _p(SEED_STEP), _s()), "vdm_gn_dyh")
    dyh.gnb_partials = channel_dot_sums(dyh, x1, x2)
    if colsum is not None and getattr(stats, "chsum", None) is None:      # the analytic column sums need sum_v x per channel
        cs = [channel_dot_sums(t, t)[:, 0, :, 0] for t in (x1, x2) if t is not None]
        stats.chsum = torch.cat(cs, dim=1).contiguous()
    _pe(ev, "gn_dyh+dot_sums", 0.0, 5.0 * dy.numel() * dy.element_size())
    out = gn_bwd_fused(x1, x2, groups, stats, gamma, dyh, dgamma, dbeta, add1=add1, add2=add2, colsum=colsum, dx1=dx1, dx2=dx2)
    if colsum is not None:                # colsum = sum_v dx INCLUDING the residual-path terms (the analytic form covers the GroupNorm part)
        if add1 is not None:
            colsum[:, :c1] += channel_dot_sums(add1, add1)[:, 0, :, 0]
        if add2 is not None:
            colsum[:, c1:c1 + c2] += channel_dot_sums(add2, add2)[:, 0, :, 0]
    return out


def gn_tail_ok(conv_in, x):
    """Can the last GroupNorm backward + conv_in's weight gradient run as one pass (gn_bwd_fused(..., tail=...))?  Where the plan of
    conv_in's weight gradient (with bias, written) is the thin-input kernel, at batch <= 16."""
    if conv_in.cout != x.shape[-1] or x.shape[0] > 16 or not FUSED_TAIL:
        return False
    info = _lib.WgradPlanInfo()
    n, od, oh, ow, _ = x.shape
    check(_lib.lib().vdm_conv_wgrad_plan(conv_in.desc(n, od, oh, ow, x.dtype), 1, 0, C.byref(info)), "vdm_conv_wgrad_plan")
    return info.kernel == _lib.WGRAD_THIN_IN


def gn_bwd_fused(x1, x2, groups, stats, gamma, dyh, dgamma, dbeta, add1=None, add2=None, colsum=None, dx1=None, dx2=None, skip=None, tail=None):
    """Second half of the GroupNorm+SiLU backward after Conv.dgrad_gn (dyh carries `.gnb_partials`).  Writes dgamma / dbeta,
    colsum (optional [N, >=C] fp32 view, row stride honoured; needs stats.chsum) and returns (dx1, dx2).  No float atomics.
    tail = (conv_in, xin, dw, dbias) (gn_tail_ok): x1 is the output of conv_in - its gradient is not written but folded straight into
    conv_in's weight / bias gradient (returns (None, None)).
    skip = (dout, w1, w2, dw1, dw2): the block's 1x1x1 skip conv rides along (gn_skip_supported(...)[1]): W^T dout is added to dx and
    the skip weight gradients dw1 / dw2 are written in the same pass (instead of add1 / add2 from a separate dgrad conv)."""
    L = _lib.lib()
    _contig(x1, x2, dyh, add1, add2, gamma, dgamma, dbeta, stats)
    n, v = _nv(x1)
    c1 = x1.shape[-1]
    c2 = 0 if x2 is None else x2.shape[-1]
    C_ = c1 + c2
    part = dyh.gnb_partials
    assert part is not None and part.shape[0] == n and part.shape[2] == C_ and dyh.shape[-1] == C_
    red = torch.empty((n, groups, 2), dtype=torch.float32, device=x1.device)
    chan = torch.empty((n, C_, 2), dtype=torch.float32, device=x1.device)
    cstride, chsum = 0, None
    if colsum is not None:
        assert colsum.dtype == torch.float32 and colsum.stride(1) == 1 and colsum.shape[0] == n
        cstride, chsum = colsum.stride(0), getattr(stats, "chsum", None)
        assert chsum is not None, "gn_bwd_fused: colsum needs the per-channel sums (gn_stats(..., chsum=True))"
    if dx1 is None and tail is None:
        dx1 = dyh if x2 is None else torch.empty_like(x1)
    if x2 is not None and dx2 is None:
        dx2 = torch.empty_like(x2)
    ev = _pb()
    check(L.vdm_gn_bwd_finalize(_p(part), part.shape[1], n, C_, groups, v, _p(stats), _p(gamma), GN_EPS, _p(chsum), _p(red), _p(chan),
                                _p(colsum), cstride, _s()), "vdm_gn_bwd_finalize")
    if tail is not None:           # the last GroupNorm of the backward pass: dx feeds only conv_in's weight gradient - never written
        conv_in, xin, dw, dbias = tail
        assert x2 is None and add2 is None and skip is None
        _contig(xin, dw, dbias, add1)
        n_, od, oh, ow, _ = x1.shape
        d = conv_in.desc(n_, od, oh, ow, x1.dtype)
        need = L.vdm_conv_wgrad_workspace_bytes(d)
        ws = _scratch(Conv._ws, (x1.device, _s()), need, torch.uint8, x1.device, floor=32 << 20)
        if "gn_apply" not in ABLATE and "wgrad" not in ABLATE:
            check(L.vdm_gn_bwd_apply_wgrad_thin(_p(x1), c1, n, od, oh, ow, groups, _p(stats), _p(gamma), GN_EPS, _p(dyh), _p(red), _p(chan), _p(add1),
                                                _p(xin), conv_in.cin, 1 if conv_in.circular else 0, _p(dgamma), _p(dbeta), _p(dw), _p(dbias), _p(ws),
                                                ws.numel(), _s()), "vdm_gn_bwd_apply_wgrad_thin")
        _pe(ev, "gn_bwd(finalize+apply)", 2.0 * n * v * 27 * conv_in.cin * c1, (2.0 + (1.0 if add1 is not None else 0.0)) * dyh.numel() * dyh.element_size())
        return None, None
    if skip is not None:
        assert add1 is None and add2 is None
        dout, w1, w2, dw1, dw2 = skip
        _contig(dout, w1, w2, dw1, dw2)
        cout = w1.shape[0]
        nws = L.vdm_gn_skip_ws_floats(c1, c2, cout, n, v)
        ws = _scratch(_skip_ws, (x1.device, _s()), nws, torch.float32, x1.device)
        if "gn_apply" not in ABLATE:
            check(L.vdm_gn_bwd_apply_skip(_p(x1), c1, _p(x2), c2, n, v, groups, dt_id(x1.dtype), _p(stats), _p(gamma), GN_EPS, _p(dyh), _p(red),
                                          _p(chan), _p(dout), _p(w1), _p(w2), cout, _p(dx1), _p(dx2), _p(dgamma), _p(dbeta), _p(dw1), _p(dw2),
                                          _p(ws), ws.numel(), _s()), "vdm_gn_bwd_apply_skip")
        _pe(ev, "gn_bwd(finalize+apply)", 4.0 * n * v * C_ * cout, (3.0 * dyh.numel() + dout.numel()) * dyh.element_size())
        return dx1, dx2
    if "gn_apply" not in ABLATE:
      check(L.vdm_gn_bwd_apply(_p(x1), c1, _p(x2), c2, n, v, groups, dt_id(x1.dtype), _p(stats), _p(gamma), GN_EPS, _p(dyh), _p(red), _p(chan),
                             _p(add1), _p(add2), _p(dx1), _p(dx2), _p(dgamma), _p(dbeta), _s()), "vdm_gn_bwd_apply")
    _pe(ev, "gn_bwd(finalize+apply)", 0.0, (3.0 + (1.0 if add1 is not None else 0.0)) * dyh.numel() * dyh.element_size())
    return dx1, dx2


def pack_input(a, b, dtype, out=None):
    """[N, D, H, W] fp32 (+ optional second channel) -> NDHWC [N, D, H, W, cpad(2)] of `dtype`, zero padded."""
    L = _lib.lib()
    _contig(a, b)
    assert a.dtype == torch.float32 and (b is None or (b.dtype == torch.float32 and b.shape == a.shape))
    cp = cpad(2, dtype)
    if out is None:
        out = torch.empty(tuple(a.shape) + (cp,), dtype=dtype, device=a.device)
    check(L.vdm_pack_input(_p(a), _p(b), a.numel(), cp, dt_id(dtype), _p(out), _s()), "vdm_pack_input")
    return out


def pack_fields(z, cond, dtype, out=None):
    """vdm_pack_fields: z [N, D, H, W] fp32 and K conditioning fields cond [N, K, D, H, W] fp32 (K in 1..3) -> conv_in's NDHWC input
    [N, D, H, W, cpad(1 + K)] = {z, c_0 .. c_{K-1}, 0...} of `dtype`: one 16-byte piece per voxel.  The kernel owns 4 voxels per thread,
    so a cube whose voxel count is no multiple of 4 is refused (ValueError) - the 3D training and sampling cubes are all even-sided."""
    L = _lib.lib()
    _contig(z, cond)
    n, per = z.shape[0], z.numel() // z.shape[0]
    assert z.dtype == cond.dtype == torch.float32 and cond.dim() == z.dim() + 1 and cond.shape[0] == n and tuple(cond.shape[2:]) == tuple(z.shape[1:])
    k = cond.shape[1]
    if per % 4:
        raise ValueError(f"pack_fields: {per} voxels per sample is not a multiple of 4")
    cp = cpad(1 + k, dtype)
    if out is None:
        out = torch.empty(tuple(z.shape) + (cp,), dtype=dtype, device=z.device)
    check(L.vdm_pack_fields(_p(z), _p(cond), k, n, per, dt_id(dtype), _p(out), _s()), "vdm_pack_fields")
    return out


class CondTable:
    """K6: the conditioning MLPs and the additive injection table of all blocks (vdm_cond_table_*).
    specs: list of dicts {input: tensor ([rows] for the sinusoidal t embedding, [rows, d] for a vector), sinusoid: bool, in_dim,
    w1, b1, w2, b2, wproj: fp32 device tensors (views into the flat parameter vector)}."""

    def __init__(self, specs, rows, width):
        self.specs, self.rows, self.width = specs, rows, width
        self.saved = None

    def _descs(self, grads=None):
        arr = (CondMlp * len(self.specs))()
        for k, sp in enumerate(self.specs):
            _contig(sp["input"], sp["w1"], sp["b1"], sp["w2"], sp["b2"], sp["wproj"])
            assert sp["input"].dtype == torch.float32 and sp["input"].shape[0] == self.rows
            d = arr[k]
            d.input, d.in_dim, d.dim, d.sinusoid = _p(sp["input"]), int(sp["in_dim"]), int(sp["w2"].shape[0]), 1 if sp["sinusoid"] else 0
            d.w1, d.b1, d.w2, d.b2, d.wproj = _p(sp["w1"]), _p(sp["b1"]), _p(sp["w2"]), _p(sp["b2"]), _p(sp["wproj"])
            assert tuple(sp["w1"].shape) == (d.dim, d.in_dim) and tuple(sp["wproj"].shape) == (self.width, d.dim)
            if grads is not None:
                g = grads[k]
                _contig(g["w1"], g["b1"], g["w2"], g["b2"], g["wproj"])
                d.dw1, d.db1, d.dw2, d.db2, d.dwproj = _p(g["w1"]), _p(g["b1"]), _p(g["w2"]), _p(g["b2"]), _p(g["wproj"])
        return arr

    def forward(self, save):
        L = _lib.lib()
        dev = self.specs[0]["w1"].device
        arr = self._descs()
        table = torch.empty((self.rows, self.width), dtype=torch.float32, device=dev)
        self.saved = torch.empty(L.vdm_cond_saved_floats(arr, len(self.specs), self.rows), dtype=torch.float32, device=dev) if save else None
        check(L.vdm_cond_table_fwd(arr, len(self.specs), self.rows, self.width, _p(table), _p(self.saved), _s()), "vdm_cond_table_fwd")
        return table

    def backward(self, dtable, grads, dbias=None, dinputs=None):
        """grads: list of dicts {w1, b1, w2, b2, wproj} of fp32 views that receive the parameter gradients (plain stores).
        dinputs (optional): one fp32 tensor or None per spec, the gradient of its input (K6i, vdm_cond_input_grad): [rows] for the
        sinusoidal t embedding (dL/dt), [rows, in_dim] for a vector conditioning."""
        L = _lib.lib()
        assert self.saved is not None and dtable.dtype == torch.float32 and dtable.stride(1) == 1 and dtable.shape[0] == self.rows
        arr = self._descs(grads)
        scratch = torch.empty(L.vdm_cond_bwd_scratch_floats(arr, len(self.specs), self.rows, self.width), dtype=torch.float32, device=dtable.device)
        check(L.vdm_cond_table_bwd(arr, len(self.specs), self.rows, self.width, _p(dtable), dtable.stride(0), _p(self.saved), _p(scratch),
                                   _p(dbias), _s()), "vdm_cond_table_bwd")
        if dinputs is not None:
            assert len(dinputs) == len(self.specs)
            for sp, d in zip(self.specs, dinputs):
                assert d is None or (d.dtype == torch.float32 and d.is_contiguous() and tuple(d.shape) == tuple(sp["input"].shape))
            ptrs = (C.c_void_p * len(self.specs))(*[_p(d) for d in dinputs])
            check(L.vdm_cond_input_grad(arr, len(self.specs), self.rows, self.width, _p(self.saved), _p(scratch), ptrs, _s()),
                  "vdm_cond_input_grad")
        self.saved = None


def cond_table_step(table_t, table_v, step_ptr, rows, width, out):
    _contig(table_t, table_v, out)
    check(_lib.lib().vdm_cond_table_step(_p(table_t), _p(table_v), _p(step_ptr), rows, width, _p(out), _s()), "vdm_cond_table_step")
    return out


def augment_batch(fields, consts, samples, crop, out=None):
    """Data path on the device (vdm_augment_batch): fields = per-channel raw cube stacks [n_sims, S, S, S] fp32 on the GPU, consts =
    per-channel (alpha, mean, std), samples = list of (sim, anchor[3], flip[3], perm[3]).  Returns the per-channel batches
    [B, 1, crop, crop, crop] fp32: periodic crop at the anchor -> (log10(x + alpha) - mean) / std -> flips -> axis permutation."""
    L = _lib.lib()
    C_, B = len(fields), len(samples)
    S = fields[0].shape[-1]
    for f in fields:
        assert f.is_cuda and f.dtype == torch.float32 and f.is_contiguous() and f.dim() == 4 and tuple(f.shape[1:]) == (S, S, S), \
            "raw fields must be contiguous fp32 [n_sims, S, S, S] tensors on the GPU"
    nsim = min(f.shape[0] for f in fields)
    if out is None:
        out = [torch.empty(B, 1, crop, crop, crop, device=fields[0].device) for _ in range(C_)]
    ch = (_lib.AugmentChannel * C_)()
    for c, (f, (alpha, mean, std)) in enumerate(zip(fields, consts)):
        _contig(out[c])
        ch[c].field, ch[c].out, ch[c].alpha, ch[c].mean, ch[c].std = f.data_ptr(), out[c].data_ptr(), float(alpha), float(mean), float(std)
    tab = (_lib.AugmentSample * B)()
    for b, (sim, anchor, flip, perm) in enumerate(samples):
        assert 0 <= int(sim) < nsim, f"simulation index {sim} out of range (0..{nsim - 1})"
        tab[b].sim = int(sim)
        for d in range(3):
            tab[b].anchor[d], tab[b].flip[d], tab[b].perm[d] = int(anchor[d]), int(bool(flip[d])), int(perm[d])
    check(L.vdm_augment_batch(ch, C_, int(S), int(crop), tab, B, _s()), "vdm_augment_batch")
    return out


def downgrid_trilinear(src, T, out=None):
    """Trilinear down-gridding on the device (vdm_downgrid_trilinear): src = cube stack [n, S, S, S] fp32 on the GPU -> [n, T, T, T] with
    the semantics of F.interpolate(src[:, None], size=T, mode="trilinear", align_corners=False), index and weight from the exact ratio."""
    assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 4 and \
        src.shape[1] == src.shape[2] == src.shape[3], "the source must be a contiguous fp32 [n, S, S, S] tensor on the GPU"
    n, S, T = src.shape[0], src.shape[-1], int(T)
    if out is None:
        out = torch.empty((n, T, T, T), dtype=torch.float32, device=src.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, T, T, T), \
        f"out must be a contiguous fp32 [{n}, {T}, {T}, {T}] tensor on the GPU"
    if n:                                                   # (an empty tensor has no storage to point at)
        check(_lib.lib().vdm_downgrid_trilinear(_p(src), _p(out), n, S, T, _s()), "vdm_downgrid_trilinear")
    return out


LOG_MOMENTS_OUT, LOG_MOMENTS_WS = 6, 12288                  # VDM_LOG_MOMENTS_OUT / _WS (doubles)


def log_moments(x, alpha, pivot):
    """Moments of v = log10(x + alpha) in float64 over a contiguous fp32 tensor on the GPU (vdm_log_moments): a dict of Python numbers
    {"n_valid", "S1" = sum(v - pivot), "S2" = sum((v - pivot)^2), "min", "max" (of the raw x), "n_bad"} over the valid elements (x finite
    and x + alpha > 0; the others are only counted, in n_bad).  Synchronises - a tool path (data.field_normalization), not the
    training path; records of several slabs taken with one pivot are merged by data.merge_log_moments."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(), "x must be a contiguous fp32 tensor on the GPU"
    n = x.numel()
    with torch.cuda.device(x.device):
        buf = torch.empty(LOG_MOMENTS_OUT + LOG_MOMENTS_WS, dtype=torch.float64, device=x.device)
        src = x if n else buf                               # (an empty tensor has no storage to point at; nothing is read)
        check(_lib.lib().vdm_log_moments(_p(src), n, float(alpha), float(pivot), _p(buf), _p(buf[LOG_MOMENTS_OUT:]), _s()),
              "vdm_log_moments")
        r = buf[:LOG_MOMENTS_OUT].tolist()
    return {"n_valid": int(r[0]), "S1": r[1], "S2": r[2], "min": r[3], "max": r[4], "n_bad": int(r[5])}


def channel_sums(x, out):
    """out[c] (fp32 view) = sum over all leading dims of x[..., c]."""
    _contig(x, out)
    c = x.shape[-1]
    check(_lib.lib().vdm_channel_sums(_p(x), x.numel() // c, c, dt_id(x.dtype), _p(out), _s()), "vdm_channel_sums")
    return out


def channel_dot_sums(a, b1, b2=None):
    """[N, 1, C, 2] fp32 = per sample and channel (sum a, sum a * b) over the voxels, b = concat(b1, b2): gnb_partials (one "tile" per
    sample) for gn_bwd_fused when the gradient a of a GroupNorm did not come out of Conv.dgrad_gn."""
    _contig(a, b1, b2)
    n, c = a.shape[0], a.shape[-1]
    c1 = b1.shape[-1]
    c2 = 0 if b2 is None else b2.shape[-1]
    assert c1 + c2 == c and b1.dtype == a.dtype and b1.shape[:-1] == a.shape[:-1]
    out = torch.empty((n, 1, c, 2), dtype=torch.float32, device=a.device)
    check(_lib.lib().vdm_channel_dot_sums(_p(a), _p(b1), c1, _p(b2), c2, n, a.numel() // (n * c), dt_id(a.dtype), _p(out), _s()),
          "vdm_channel_dot_sums")
    return out


def attn_split_heads(src, sub, nsub, heads, rowmajor=True, transposed=True):
    """src: [N, ..., nsub * C] activations (sub-tensor `sub` of nsub: the q / k / v of the qkv conv, or nsub = 1) -> (row-major
    [N, H, V, hd], transposed [N, H, hd, V]) in src's dtype (either None when not requested)."""
    _contig(src)
    N = src.shape[0]
    C = src.shape[-1] // nsub
    V = src.numel() // (N * nsub * C)
    hd = C // heads
    rm = torch.empty((N, heads, V, hd), dtype=src.dtype, device=src.device) if rowmajor else None
    tr = torch.empty((N, heads, hd, V), dtype=src.dtype, device=src.device) if transposed else None
    check(_lib.lib().vdm_attn_split_heads(_p(src), nsub * C, sub * C, N, V, heads, hd, dt_id(src.dtype), _p(rm), _p(tr), _s()), "vdm_attn_split_heads")
    return rm, tr


def attn_fwd(q, k, vt, scale, out_shape, want_lse=True):
    """q, k: [N, H, V, hd]; vt: [N, H, hd, V] -> out (out_shape = [N, ..., H*hd], the NDHWC tensor the projection conv reads), lse [N, H, V]."""
    _contig(q, k, vt)
    N, H, V, hd = q.shape
    out = torch.empty(out_shape, dtype=q.dtype, device=q.device)
    lse = torch.empty((N, H, V), dtype=torch.float32, device=q.device) if want_lse else None
    check(_lib.lib().vdm_attn_fwd(_p(q), _p(k), _p(vt), N, V, H, hd, dt_id(q.dtype), float(scale), _p(out), _p(lse), _s()), "vdm_attn_fwd")
    return out, lse


def attn_bwd(q, k, v, qt, kt, dout, out, lse, scale, dsum=None):
    """-> dqkv [N, ..., 3 * H*hd] (the gradient of the qkv conv's output).  dout / out: [N, ..., H*hd].  dsum: [N, H, V] fp32 used in
    place of rowsum(dout * out) (then `out` is not read and may be None); the kernel tests supply integers there."""
    _contig(q, k, v, qt, kt, dout, out, lse, dsum)
    N, H, V, hd = q.shape
    L = _lib.lib()
    doh, dot = attn_split_heads(dout, 0, 1, H)
    if dsum is None:
        dsum = torch.empty((N, H, V), dtype=torch.float32, device=q.device)
        check(L.vdm_attn_rowdot(_p(dout), _p(out), N, V, H, hd, dt_id(q.dtype), _p(dsum), _s()), "vdm_attn_rowdot")
    else:
        assert dsum.dtype == torch.float32 and tuple(dsum.shape) == (N, H, V) and dsum.device == q.device
    dqkv = torch.empty(tuple(dout.shape[:-1]) + (3 * H * hd,), dtype=q.dtype, device=q.device)
    check(L.vdm_attn_bwd(_p(q), _p(k), _p(v), _p(qt), _p(kt), _p(doh), _p(dot), _p(lse), _p(dsum), N, V, H, hd, dt_id(q.dtype), float(scale),
                         _p(dqkv), _s()), "vdm_attn_bwd")
    return dqkv


def diffuse(x, eps, alpha, sigma, out=None):
    L = _lib.lib()
    _contig(x, eps, alpha, sigma)
    n = x.shape[0]
    if out is None:
        out = torch.empty_like(x)
    check(L.vdm_diffuse(_p(x), _p(eps), _p(alpha), _p(sigma), n, x.numel() // n, _p(out), _s()), "vdm_diffuse")
    return out


def _head_outputs(who, x, channels, dtype, want_z, z_out=None, packed_out=None):
    """What the fused heads share: x [N, 1, D, H, W] (or [N, D, H, W]) fp32 -> (n, per, spatial shape, z fp32 or None, packed
    [N, D, H, W, cpad(channels)] of `dtype`).  z_out / packed_out are validated and used instead of fresh tensors (z_out implies want_z).
    The kernel owns 4 voxels per thread: a sample whose voxel count is no multiple of 4 is refused (ValueError)."""
    n = x.shape[0]
    per = x.numel() // n
    if per % 4:
        raise ValueError(f"{who}: {per} voxels per sample is not a multiple of 4")
    assert x.dtype == torch.float32
    sp = tuple(x.shape[2:]) if x.dim() == 5 else tuple(x.shape[1:])
    packed = packed_out if packed_out is not None else torch.empty((n,) + sp + (cpad(channels, dtype),), dtype=dtype, device=x.device)
    assert packed.dtype == dtype and packed.numel() == x.numel() * cpad(channels, dtype)
    z = z_out if z_out is not None else (torch.empty_like(x) if want_z else None)
    assert z is None or (z.dtype == torch.float32 and z.numel() == x.numel())
    return n, per, sp, z, packed


def _check_keep(who, keep, n):
    assert keep.dtype == torch.float32 and keep.numel() == n and keep.is_contiguous(), f"{who}: keep must be {n} contiguous fp32 values"


def cond_keep(p, seed, rows, device, row0=0, out=None):
    """The per-row keep of conditioning dropout (vdm_cond_keep): [rows] fp32 {0, 1}, row r kept iff the uniform draw of GLOBAL row
    row0 + r - Philox keyed by `seed` (mixed with SEED_STEP inside the kernel when a captured step set it) - exceeds p."""
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=device)
    _check_keep("cond_keep", out, rows)
    check(_lib.lib().vdm_cond_keep(float(p), int(seed), _p(SEED_STEP), int(row0), rows, _p(out), _s()), "vdm_cond_keep")
    return out


def mask_rows(v, keep, out=None):
    """vdm_mask_rows: out[r] = v[r] where keep[r] != 0, +0 elsewhere (a select: NaN / Inf of a dropped row do not get through).
    v: fp32 [rows, ...]; out may be v."""
    _contig(v, out)
    assert v.dtype == torch.float32
    rows = v.shape[0]
    _check_keep("mask_rows", keep, rows)
    if out is None:
        out = torch.empty_like(v)
    assert out.dtype == torch.float32 and out.shape == v.shape
    check(_lib.lib().vdm_mask_rows(_p(v), _p(keep), rows, v.numel() // rows, _p(out), _s()), "vdm_mask_rows")
    return out


def diffuse_pack(x, s_cond, alpha, sigma, dtype, eps=None, seed=0, stream_id=0, want_z=False, z_out=None, packed_out=None, keep_s=None):
    """Fused head of the training step (vdm_diffuse_pack): z_t = alpha[n] x + sigma[n] eps -> (z_t fp32 or None, conv_in's NDHWC input
    [N, D, H, W, cpad(2)] = {z_t, s_cond, 0...} in `dtype`).  eps None: drawn inside the kernel from Philox(seed, stream_id) - the field
    randn(out, seed, stream_id) would have written.  z_out / packed_out: write there instead of into fresh tensors (z_out implies want_z).
    keep_s ([N] fp32, needs s_cond): rows with keep_s == 0 get +0 instead of s_cond, which is not read there
    (vdm_diffuse_pack_fields_keep with k = 1: the same bits)."""
    n, per, _, z, packed = _head_outputs("diffuse_pack", x, 2, dtype, want_z, z_out, packed_out)
    L = _lib.lib()
    _contig(x, s_cond, eps, alpha, sigma, z_out, packed_out)
    assert s_cond is None or (s_cond.shape == x.shape and s_cond.dtype == torch.float32)
    if keep_s is not None and s_cond is not None:
        _check_keep("diffuse_pack", keep_s, n)
        check(L.vdm_diffuse_pack_fields_keep(_p(x), _p(s_cond), 1, _p(eps), int(seed), int(stream_id), _p(SEED_STEP), _p(alpha), _p(sigma), n,
                                             per, dt_id(dtype), _p(z), _p(packed), _p(keep_s), _s()), "vdm_diffuse_pack_fields_keep")
        return z, packed
    check(L.vdm_diffuse_pack(_p(x), _p(s_cond), _p(eps), int(seed), int(stream_id), _p(SEED_STEP), _p(alpha), _p(sigma), n, per, dt_id(dtype),
                             _p(z), _p(packed), _s()), "vdm_diffuse_pack")
    return z, packed


def diffuse_pack_fields(x, cond, alpha, sigma, dtype, eps=None, seed=0, stream_id=0, want_z=False, keep_s=None):
    """diffuse_pack for K conditioning fields (vdm_diffuse_pack_fields): x [N, 1, D, H, W] (or [N, D, H, W]), cond [N, K, D, H, W], K in
    1..3 -> (z_t fp32 or None, packed [N, D, H, W, cpad(1 + K)] = {z_t, c_0 .. c_{K-1}, 0...}).  The noise is keyed as in diffuse_pack:
    z_t and channel 0 are the bits diffuse_pack gives for the same arguments.  keep_s ([N] fp32): rows with keep_s == 0 get +0 in all
    K planes and their cond is not read (vdm_diffuse_pack_fields_keep)."""
    k = cond.shape[1]
    n, per, sp, z, packed = _head_outputs("diffuse_pack_fields", x, 1 + k, dtype, want_z)
    L = _lib.lib()
    _contig(x, cond, eps, alpha, sigma)
    assert cond.dtype == torch.float32 and cond.shape[0] == n and tuple(cond.shape[2:]) == sp
    if keep_s is not None:
        _check_keep("diffuse_pack_fields", keep_s, n)
        check(L.vdm_diffuse_pack_fields_keep(_p(x), _p(cond), k, _p(eps), int(seed), int(stream_id), _p(SEED_STEP), _p(alpha), _p(sigma), n,
                                             per, dt_id(dtype), _p(z), _p(packed), _p(keep_s), _s()), "vdm_diffuse_pack_fields_keep")
        return z, packed
    check(L.vdm_diffuse_pack_fields(_p(x), _p(cond), k, _p(eps), int(seed), int(stream_id), _p(SEED_STEP), _p(alpha), _p(sigma), n, per,
                                    dt_id(dtype), _p(z), _p(packed), _s()), "vdm_diffuse_pack_fields")
    return z, packed


def _k1t(entry, dh, weight, cin, circular, ds_planes, tail=()):
    """What the two K1t entries share: dh NDHWC [N, D, H, W, C], conv_in's fp32 master weight [27, C, cin] -> (dz [N, D, H, W], ds
    [N, *ds_planes, D, H, W] or None when ds_planes is None), fp32.  tail: the entry's arguments between ds and the stream."""
    L = _lib.lib()
    _contig(dh, weight)
    n, d, h, w, c = dh.shape
    assert weight.dtype == torch.float32 and tuple(weight.shape) == (27, c, cin)
    dz = torch.empty((n, d, h, w), dtype=torch.float32, device=dh.device)
    ds = torch.empty((n,) + ds_planes + (d, h, w), dtype=torch.float32, device=dh.device) if ds_planes is not None else None
    check(getattr(L, entry)(_p(dh), n, d, h, w, c, dt_id(dh.dtype), _lib.PAD_CIRCULAR if circular else _lib.PAD_ZEROS, _p(weight), cin,
                            _p(dz), _p(ds), *tail, _s()), entry)
    return dz, ds


def conv_in_dgrad_fields(dh, weight, cin, circular, want_s):
    """K1t for cin = 1 + K in 1..4 (vdm_conv_in_dgrad_fields): (dz [N, D, H, W], ds [N, K, D, H, W] or None) fp32 from dh (NDHWC
    [N, D, H, W, C]) and conv_in's fp32 master weight [27, C, cin].  want_s False: dz alone (n_ds = 0)."""
    n_ds = cin - 1 if want_s else 0
    return _k1t("vdm_conv_in_dgrad_fields", dh, weight, cin, circular, (n_ds,) if n_ds else None, (n_ds,))


def conv_in_dgrad(dh, weight, cin, circular, want_s):
    """K1t (vdm_conv_in_dgrad): the gradient of conv_in's input channels from dh = d loss / d conv_in output (NDHWC [N, D, H, W, C]).
    weight: conv_in's fp32 master weight [27, C, cin].  Returns (dz, ds or None), fp32 [N, D, H, W]."""
    return _k1t("vdm_conv_in_dgrad", dh, weight, cin, circular, () if want_s else None)


def schedule_grad_sums(dz, x, eps=None, seed=0, stream_id=0):
    """K7b (vdm_schedule_grad_sums): [N, 2] fp32 = (sum dz x, sum dz eps) per sample; eps None: regenerated from Philox(seed, stream_id) -
    the field diffuse_pack(..., seed, stream_id) drew."""
    L = _lib.lib()
    _contig(dz, x, eps)
    n = x.shape[0]
    assert dz.shape == x.shape and dz.dtype == x.dtype == torch.float32 and (eps is None or eps.shape == x.shape)
    out = torch.empty((n, 2), dtype=torch.float32, device=x.device)
    check(L.vdm_schedule_grad_sums(_p(dz), _p(x), _p(eps), int(seed), int(stream_id), _p(SEED_STEP), n, x.numel() // n, _p(out),
                                   _p(_reduce_ws(x.device)), _s()), "vdm_schedule_grad_sums")
    return out


_red_ws = {}


def _reduce_ws(device):
    """per-(device, stream) scratch of the fixed-order two-stage reductions (loss terms, gradient norm)"""
    return _scratch(_red_ws, (device, _s()), 2048 * 3, torch.float32, device)


def loss_terms(x, eps, eps_hat, eps0, sigma0_over_alpha0, coef, sums, d_eps_hat, rng=None, workspace=None):
    """K8.  rng = ((seed_eps, stream_eps), (seed_eps0, stream_eps0)): a noise field passed as None is regenerated inside the kernel from
    its Philox counters (vdm_loss_terms_rng) instead of read.  workspace: the caller's 2048 * 3 floats instead of the cached scratch."""
    L = _lib.lib()
    ws = workspace if workspace is not None else _reduce_ws(x.device)
    assert ws.dtype == torch.float32 and ws.numel() >= 2048 * 3
    _contig(x, eps, eps_hat, eps0, coef, sums, d_eps_hat)
    n = x.shape[0]
    per = x.numel() // n
    if per % 4 == 0 and (rng is not None or (eps is not None and eps0 is not None)):      # vector kernel (also for supplied fields: one
        (se, ie), (s0, i0) = rng if rng is not None else ((0, 0), (0, 0))                   # summation order for both forms)
        assert rng is not None or (eps is not None and eps0 is not None)
        check(L.vdm_loss_terms_rng(_p(x), _p(eps), int(se), int(ie), _p(eps_hat), _p(eps0), int(s0), int(i0), _p(SEED_STEP),
                                   float(sigma0_over_alpha0), _p(coef), n, per, _p(sums), _p(d_eps_hat), _p(ws), _s()),
              "vdm_loss_terms_rng")
        return
    assert eps is not None and eps0 is not None, "loss_terms: noise fields missing (and no Philox counters to regenerate them from)"
    check(L.vdm_loss_terms(_p(x), _p(eps), _p(eps_hat), _p(eps0), float(sigma0_over_alpha0), _p(coef), n, per,
                           _p(sums), _p(d_eps_hat), _p(ws), _s()), "vdm_loss_terms")


def sfm_head(x0, x1, t, sigma, dtype, cond=True, eps=None, seed=0, stream_id=0, want_x=False, x_out=None, packed_out=None):
    """Fused head of the flow-matching step (vdm_sfm_head): x_t = (1 - t[n]) x0 + t[n] x1 (+ sigma eps when sigma > 0) -> (x_t fp32 or
    None, conv_in's NDHWC input [N, D, H, W, cpad(2)] = {x_t, x0 if cond else 0, 0...} in `dtype`).  eps None with sigma > 0: drawn inside
    the kernel from Philox(seed, stream_id) - the field randn(out, seed, stream_id) would have written; sigma == 0: no noise is read or
    drawn.  x_out / packed_out: write there instead of into fresh tensors (x_out implies want_x).  The kernel owns 4 voxels per thread:
    a sample whose voxel count is no multiple of 4 is refused (ValueError)."""
    n, per, _, x_t, packed = _head_outputs("sfm_head", x0, 2, dtype, want_x, x_out, packed_out)
    L = _lib.lib()
    _contig(x0, x1, t, eps, x_out, packed_out)
    assert x1.dtype == t.dtype == torch.float32 and x1.shape == x0.shape and t.numel() == n
    assert eps is None or (eps.dtype == torch.float32 and eps.shape == x0.shape)
    check(L.vdm_sfm_head(_p(x0), _p(x1), _p(eps), int(seed), int(stream_id), _p(SEED_STEP), _p(t), float(sigma), int(bool(cond)), n, per,
                         dt_id(dtype), _p(x_t), _p(packed), _s()), "vdm_sfm_head")
    return x_t, packed


def sfm_loss(v_hat, x0, x1, coef, sums, d_v, workspace=None):
    """Flow-matching loss (vdm_sfm_loss): sums[n] += sum (v_hat - (x1 - x0))^2, d_v = coef[n] (v_hat - (x1 - x0)); the target field is never
    written.  sums: [N] fp32, zeroed by the caller.  workspace: the caller's 2048 * 3 floats instead of the cached scratch.  A sample whose
    element count is no multiple of 4 is refused (ValueError).  (No generator is involved: SEED_STEP has nothing to reach here.)"""
    n = x0.shape[0]
    per = x0.numel() // n
    if per % 4:
        raise ValueError(f"sfm_loss: {per} elements per sample is not a multiple of 4")
    L = _lib.lib()
    ws = workspace if workspace is not None else _reduce_ws(x0.device)
    assert ws.dtype == torch.float32 and ws.numel() >= 2048 * 3
    _contig(v_hat, x0, x1, coef, sums, d_v)
    assert v_hat.dtype == x0.dtype == x1.dtype == coef.dtype == sums.dtype == d_v.dtype == torch.float32
    assert v_hat.numel() == x0.numel() == x1.numel() == d_v.numel() and coef.numel() == n and sums.numel() == n
    check(L.vdm_sfm_loss(_p(v_hat), _p(x0), _p(x1), _p(coef), n, per, _p(sums), _p(d_v), _p(ws), _s()), "vdm_sfm_loss")


def ancestral_step(z, eps_hat, noise, coef, step_ptr, seed, eps_uncond=None, w_cfg=0.0):
    """K9.  eps_uncond given: classifier-free guidance, (1 + w_cfg) * eps_hat - w_cfg * eps_uncond blended inside the update."""
    L = _lib.lib()
    _contig(z, eps_hat, noise, coef, eps_uncond)
    if eps_uncond is None:
        check(L.vdm_ancestral_step(_p(z), _p(eps_hat), _p(noise), _p(coef), _p(step_ptr), int(seed), z.numel(), _s()),
              "vdm_ancestral_step")
    else:
        assert eps_uncond.shape == eps_hat.shape == z.shape and eps_uncond.dtype == torch.float32
        check(L.vdm_ancestral_step_cfg(_p(z), _p(eps_hat), _p(eps_uncond), float(w_cfg), _p(noise), _p(coef), _p(step_ptr), int(seed),
                                       z.numel(), _s()), "vdm_ancestral_step_cfg")


def ancestral_step_rows(z, eps_hat, coef, step_ptr, seeds_dev, eps_uncond=None, w_cfg=0.0):
    """K9, row-keyed: row r of z ([rows, ...]) draws its noise from seeds_dev[r] (a device int64 tensor of `rows` seeds), so a chain's
    noise is the same in any batch; rows == 1 gives ancestral_step(seed=seeds_dev[0]) bit for bit.  eps_uncond: the w_cfg blend."""
    L = _lib.lib()
    _contig(z, eps_hat, coef, eps_uncond, seeds_dev)
    rows = z.shape[0]
    assert eps_hat.shape == z.shape and z.dtype == eps_hat.dtype == torch.float32
    assert eps_uncond is None or (eps_uncond.shape == z.shape and eps_uncond.dtype == torch.float32)
    assert seeds_dev.dtype == torch.int64 and seeds_dev.numel() == rows and seeds_dev.device == z.device
    check(L.vdm_ancestral_step_rows(_p(z), _p(eps_hat), _p(eps_uncond), float(w_cfg), _p(coef), _p(step_ptr), _p(seeds_dev), rows,
                                    z.numel() // rows, _s()), "vdm_ancestral_step_rows")


def multistep_step(z, eps_hat, prev, coef, step_ptr, eps_uncond=None, w_cfg=0.0):
    """K9m: est = e_z z + e_e e, z <- w_z z + w_x est + w_p prev, prev <- est, the scalars from row *step_ptr of coef [steps, 8] fp32 =
    {e_z, e_e, w_z, w_x, w_p, t_net, 0, 0}; a row with w_p == 0 does not read prev.  eps_uncond: the w_cfg blend of K9."""
    L = _lib.lib()
    _contig(z, eps_hat, prev, coef, eps_uncond)
    assert eps_hat.shape == prev.shape == z.shape and z.dtype == eps_hat.dtype == prev.dtype == coef.dtype == torch.float32
    assert eps_uncond is None or (eps_uncond.shape == z.shape and eps_uncond.dtype == torch.float32)
    assert coef.dim() == 2 and coef.shape[1] == 8 and step_ptr.dtype == torch.int32
    check(L.vdm_multistep_step(_p(z), _p(eps_hat), _p(eps_uncond), float(w_cfg), _p(prev), _p(coef), _p(step_ptr), z.numel(), _s()),
          "vdm_multistep_step")


class DdnmTables:
    """The device tables behind the DDNM kernels (vdm_ddnm_tables): coef [n, 8] fp32 = {1/alpha_t, sigma_t, w_z, w_x, scale, t_norm, 0, 0},
    sched [n_sched, 2] int32 = {grid index k, draw number} per network evaluation, cursor int32 [1] (the evaluation index), k_ptr int32
    [1] (the k of the current evaluation: what cond_table_step reads), seeds int64 [rows] or None (every launch gets a noise field);
    batch_stream: one Philox stream over the whole batch from seeds[0] instead of one per row."""

    def __init__(self, coef, sched, seeds=None, batch_stream=False):
        dev = coef.device
        assert coef.dtype == torch.float32 and coef.dim() == 2 and coef.shape[1] == 8 and sched.dtype == torch.int32 and sched.shape[1] == 2
        assert seeds is None or (seeds.dtype == torch.int64 and seeds.device == dev)
        _contig(coef, sched, seeds)
        self.coef, self.sched, self.seeds = coef, sched, seeds
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.k_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
        self.c = _lib.DdnmTables(coef=coef.data_ptr(), sched=sched.data_ptr(), cursor=self.cursor.data_ptr(), n_coef=coef.shape[0],
                                 n_sched=sched.shape[0], seeds=None if seeds is None else seeds.data_ptr(),
                                 batch_stream=int(bool(batch_stream)), reserved=0)
        self.reset()

    def reset(self, e=0):
        """Cursor to evaluation e (device-side copies: no host synchronisation)."""
        self.cursor.fill_(e)
        self.k_ptr.copy_(self.sched[e, :1])

    def advance(self):
        check(_lib.lib().vdm_ddnm_advance(_p(self.cursor), _p(self.sched), self.sched.shape[0], _p(self.k_ptr), _s()), "vdm_ddnm_advance")

    def _ref(self):
        _p(self.coef), _p(self.sched), _p(self.cursor), _p(self.seeds)       # (side-stream bookkeeping of _p)
        return C.byref(self.c)


def _ddnm_rows(z, *same):
    rows = z.shape[0]
    assert z.dtype == torch.float32
    for t in same:
        assert t is None or (t.shape == z.shape and t.dtype == torch.float32), "DDNM fields must be fp32 tensors of z's shape"
    return rows, z.numel() // rows


def ddnm_x0(z, eps_hat, tables, out, eps_uncond=None, w_cfg=0.0):
    """x_0t = (z - sigma_t eps_hat) / alpha_t at the cursor's grid index; eps_uncond: the w_cfg blend of K9."""
    _contig(z, eps_hat, eps_uncond, out)
    _ddnm_rows(z, eps_hat, eps_uncond, out)
    check(_lib.lib().vdm_ddnm_x0(_p(z), _p(eps_hat), _p(eps_uncond), float(w_cfg), tables._ref(), _p(out), z.numel(), _s()), "vdm_ddnm_x0")
    return out


def ddnm_update(z, x0, atax0, aty, tables, noise=None, x_r=None):
    """x_r = (aty + x0) - atax0 ; z <- w_z z + w_x x_r + scale noise (in place).  aty: z's shape or one row.  x_r None: not written."""
    _contig(z, x0, atax0, aty, noise, x_r)
    rows, per = _ddnm_rows(z, x0, atax0, noise, x_r)
    assert aty.dtype == torch.float32 and aty.numel() in (per, rows * per)
    check(_lib.lib().vdm_ddnm_update(_p(z), _p(x0), _p(atax0), _p(aty), aty.numel() // per, _p(noise), tables._ref(), _p(x_r), rows, per,
                                     _s()), "vdm_ddnm_update")


def ddnm_mask_step(z, eps_hat, mask, y, tables, noise=None, x_r=None, eps_uncond=None, w_cfg=0.0):
    """The whole DDNM evaluation tail for A = AT = mask in one launch.  mask / y: z's shape or one row of it."""
    _contig(z, eps_hat, eps_uncond, mask, y, noise, x_r)
    rows, per = _ddnm_rows(z, eps_hat, eps_uncond, noise, x_r)
    assert mask.dtype == y.dtype == torch.float32 and mask.numel() in (per, rows * per) and y.numel() in (per, rows * per)
    check(_lib.lib().vdm_ddnm_mask_step(_p(z), _p(eps_hat), _p(eps_uncond), float(w_cfg), _p(mask), mask.numel() // per, _p(y),
                                        y.numel() // per, _p(noise), tables._ref(), _p(x_r), rows, per, _s()), "vdm_ddnm_mask_step")


def ddnm_blockmean_step(z, eps_hat, y, factors, tables, noise=None, x_r=None, eps_uncond=None, w_cfg=0.0):
    """The whole DDNM evaluation tail for A = mean over factors = (fz, fy, fx) blocks, AT = nearest up-sampling, in one launch.
    z is [rows, C, D, H, W] (the channels fold into the z axis); y is [rows or 1, C, D/fz, H/fy, W/fx]."""
    _contig(z, eps_hat, eps_uncond, y, noise, x_r)
    rows, per = _ddnm_rows(z, eps_hat, eps_uncond, noise, x_r)
    fz, fy, fx = (int(f) for f in factors)
    d, h, w = z.shape[-3] * (per // (z.shape[-3] * z.shape[-2] * z.shape[-1])), z.shape[-2], z.shape[-1]
    nblk = fz * fy * fx
    assert y.dtype == torch.float32 and y.numel() * nblk in (per, rows * per), "y must hold one value per block"
    check(_lib.lib().vdm_ddnm_blockmean_step(_p(z), _p(eps_hat), _p(eps_uncond), float(w_cfg), _p(y), y.numel() * nblk // per, d, h, w, fz,
                                             fy, fx, _p(noise), tables._ref(), _p(x_r), rows, _s()), "vdm_ddnm_blockmean_step")


def ddnm_travel(z, tables, travel, outer, draw, noise=None):
    """z <- a z + b noise with {a, b} = travel[outer] (device table [n, 2]); Philox draw number `draw`, or the supplied field."""
    _contig(z, noise, travel)
    rows, per = _ddnm_rows(z, noise)
    assert travel.dtype == torch.float32 and 0 <= outer < travel.shape[0]
    check(_lib.lib().vdm_ddnm_travel(_p(z), _p(noise), tables._ref(), _p(travel), int(outer), int(draw), rows, per, _s()), "vdm_ddnm_travel")


def randn(out, seed, stream_id=0):
    L = _lib.lib()
    _contig(out)
    assert out.dtype == torch.float32
    check(L.vdm_randn(_p(out), out.numel(), int(seed), int(stream_id), _p(SEED_STEP), _s()), "vdm_randn")
    return out


def step_inc(step_ptr):
    check(_lib.lib().vdm_step_inc(_p(step_ptr), _s()), "vdm_step_inc")


def ema_update(ema, p, decay, warmup=True, num_updates=None):
    """vdm_ema_update: ema += (1 - d_k) * (p - ema) with d_k = min(decay, (1 + k) / (10 + k)) under warmup, k = num_updates[0] read on the
    device (None: 0).  Contiguous fp32 tensors of equal size, any 4-byte alignment.  The counter is not bumped (step_inc)."""
    _contig(ema, p, num_updates)
    assert ema.dtype == torch.float32 and p.dtype == torch.float32 and ema.numel() == p.numel(), "ema_update: two fp32 tensors of one size"
    assert num_updates is None or (num_updates.dtype == torch.int32 and num_updates.numel() >= 1)
    check(_lib.lib().vdm_ema_update(_p(ema), _p(p), ema.numel(), float(decay), int(bool(warmup)), _p(num_updates), _s()), "vdm_ema_update")
    return ema


def swap_(a, b):
    """vdm_swap: exchanges the contents of two contiguous fp32 tensors of equal size in place (no temporary)."""
    _contig(a, b)
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.numel() == b.numel(), "swap_: two fp32 tensors of one size"
    check(_lib.lib().vdm_swap(_p(a), _p(b), a.numel(), _s()), "vdm_swap")


def sumsq(x, out, workspace=None):
    """out[0] += sum x^2.  workspace: the caller's 2048 floats instead of the cached scratch."""
    L = _lib.lib()
    _contig(x)
    assert x.dtype == torch.float32 and out.dtype == torch.float32
    ws = workspace if workspace is not None else _reduce_ws(x.device)
    assert ws.dtype == torch.float32 and ws.numel() >= 2048
    check(L.vdm_sumsq(_p(x), x.numel(), _p(out), _p(ws), _s()), "vdm_sumsq")
    return out


def train_scalars(B, device, rank, world, gamma_min, gamma_max, bpd_over_B, u0=None, times=None, seed=0):
    """[5, B] fp32 = {t, alpha_t, sigma_t, coef, t_norm} (vdm_train_scalars); u0: device tensor with one uniform draw, or times [B];
    neither: u0 is drawn inside the kernel from (seed, SEED_STEP) - the graph-captured training step."""
    out = torch.empty((5, B), dtype=torch.float32, device=device)
    _contig(u0, times)
    check(_lib.lib().vdm_train_scalars(_p(u0), _p(times), B, rank, world, float(gamma_min), float(gamma_max), float(bpd_over_B), _p(out),
                                       int(seed), _p(SEED_STEP), _s()), "vdm_train_scalars")
    return out


def elbo_assemble(sums, coef, c_lat0, c_lat1, c_rec0, c_rec1):
    _contig(sums, coef)
    out = torch.empty(4, dtype=torch.float32, device=sums.device)
    check(_lib.lib().vdm_elbo_assemble(_p(sums), _p(coef), sums.shape[0], float(c_lat0), float(c_lat1), float(c_rec0), float(c_rec1), _p(out), _s()),
          "vdm_elbo_assemble")
    return out


def clip_scale_(x, sumsq_acc, max_norm):
    _contig(x)
    check(_lib.lib().vdm_clip_scale(_p(x), x.numel(), _p(sumsq_acc), float(max_norm), _s()), "vdm_clip_scale")
    return x


class PackPlan:
    """All (conv, form) weight packings of a network as one launch (vdm_conv_pack_many): the item and chunk tables are built
    once per (parameter storage, dtype, forms) and live on the device."""

    def __init__(self, convs_and_masters, dtype, need_dgrad):
        """convs_and_masters: [(Conv, fp32 master view [taps, cout, cin] inside the flat parameter vector)]."""
        import numpy as np
        L = _lib.lib()
        device = convs_and_masters[0][1].device
        items = []
        for conv, w in convs_and_masters:
            assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() == conv.ksize ** 3 * conv.cout * conv.cin
            conv.alloc_packed(device, dtype, need_dgrad)
            d = conv.desc(1, 2, 2, 2, dtype)
            for mode, buf in ((PACK_FWD, conv.wf),) + (((PACK_DGRAD, conv.wd),) if need_dgrad else ()):
                it = _lib.PackItem()
                check(L.vdm_conv_pack_plan(d, mode, _p(w), _p(buf), C.byref(it)), "vdm_conv_pack_plan")
                items.append(it)
        chunks = []
        for i, it in enumerate(items):
            for first in range(0, it.elems, _lib.PACK_CHUNK):
                chunks.append((i, min(_lib.PACK_CHUNK, it.elems - first), first))
        item_arr = (_lib.PackItem * len(items))(*items)
        chunk_arr = (_lib.PackChunk * len(chunks))(*[_lib.PackChunk(*c) for c in chunks])
        self.items = torch.from_numpy(np.frombuffer(bytes(item_arr), dtype=np.uint8).copy()).to(device)
        self.chunks = torch.from_numpy(np.frombuffer(bytes(chunk_arr), dtype=np.uint8).copy()).to(device)
        self.nchunks = len(chunks)
        self.dtype = dtype

    def run(self):
        if "pack" in ABLATE and getattr(self, "_ran", False):
            return
        self._ran = True
        check(_lib.lib().vdm_conv_pack_many(_p(self.items), _p(self.chunks), self.nchunks, dt_id(self.dtype), _s()), "vdm_conv_pack_many")
