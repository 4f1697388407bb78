"""vdm_ema_update and vdm_swap on the GPU against tests/_ema_ref.py: bit for bit against the numpy float32 recurrence, within the derived
bounds of the float64 one, over every size / alignment / counter / flag / decay the code paths distinguish; canaries around both
buffers; the update and its counter bump captured in a graph and replayed."""
import functools

import numpy as np
import pytest
import torch

import _ema_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


class Vec:
    """n floats on the device with PAD canary words on both sides; off = 1 moves the vector off the 16-byte grid by one float."""

    def __init__(self, n, off):
        self.n, self.start = n, R.PAD + off
        self.words = torch.full((R.PAD + 1 + n + R.PAD,), R.CANARY, dtype=torch.int32, device=DEV)
        self.t = self.words.view(torch.float32)[self.start:self.start + n]
        assert self.t.data_ptr() % 16 == (4 if off else 0) and self.t.is_contiguous()

    def put(self, src):
        self.t.copy_(src)
        return self

    def get(self):
        return self.t.cpu().numpy()

    def canaries_intact(self):
        w = self.words.cpu().numpy()
        return bool((w[:self.start] == R.CANARY).all() and (w[self.start + self.n:] == R.CANARY).all())


@functools.lru_cache(maxsize=None)
def reference(n, decay, warm, k):
    """(float32 reference, is it within both float64 bounds) for the shared inputs of size n - computed once for the three alignments."""
    e, p = R.inputs(n)
    ref = R.ema_step(e, p, decay, warm, k)
    err = np.abs(ref.astype(np.float64) - R.ema_step64(e, p, decay, warm, k))
    return ref, bool((err <= R.bound(e, p, ref, decay, warm, k)).all() and (err <= R.bound_max(e, p, ref, decay, warm, k)).all())


def offsets(alignment):
    return {"aligned": (0, 0), "ema_off1": (1, 0), "p_off1": (0, 1)}[alignment]


@pytest.mark.parametrize("alignment", R.ALIGNMENTS)
@pytest.mark.parametrize("n", R.SIZES)
def test_ema_update_matches_the_float32_reference_bit_for_bit(n, alignment):
    from vdm4cdm_amd import hip_ops as ops
    e_np, p_np = R.inputs(n)
    e_dev, p_dev = torch.from_numpy(e_np.copy()).to(DEV), torch.from_numpy(p_np.copy()).to(DEV)
    oe, op = offsets(alignment)
    ema, par = Vec(n, oe), Vec(n, op).put(p_dev)
    same = bits(e_np) == bits(p_np)
    assert same.any() or n < 4
    for decay in R.DECAYS:
        for warm in (True, False):
            for k in R.COUNTERS:
                ema.put(e_dev)
                counter = None if k is None else torch.tensor([k], dtype=torch.int32, device=DEV)
                ops.ema_update(ema.t, par.t, decay, warm, counter)
                got = ema.get()
                ref, within = reference(n, decay, warm, k or 0)
                bad = bits(got) != bits(ref)
                assert not bad.any(), f"decay {decay} warmup {warm} k {k}: {bad.sum()} of {n} values differ, first at {np.flatnonzero(bad)[:4]}"
                assert within                                   # got IS ref, so the float64 bounds of _ema_ref hold for the kernel's output
                assert np.array_equal(bits(got[same]), bits(e_np[same]))          # p == e leaves e untouched
                assert counter is None or counter.item() == k                    # the kernel does not bump the counter
    assert np.array_equal(bits(par.get()), bits(p_np))
    assert ema.canaries_intact() and par.canaries_intact()


@pytest.mark.parametrize("alignment", R.ALIGNMENTS)
@pytest.mark.parametrize("n", R.SIZES)
def test_swap_exchanges_exactly_and_twice_restores(n, alignment):
    from vdm4cdm_amd import hip_ops as ops
    a_np, b_np = R.inputs(n)
    oa, ob = offsets(alignment)
    a, b = Vec(n, oa).put(torch.from_numpy(a_np.copy()).to(DEV)), Vec(n, ob).put(torch.from_numpy(b_np.copy()).to(DEV))
    ops.swap_(a.t, b.t)
    assert np.array_equal(bits(a.get()), bits(b_np)) and np.array_equal(bits(b.get()), bits(a_np))
    assert a.canaries_intact() and b.canaries_intact()
    ops.swap_(a.t, b.t)
    assert np.array_equal(bits(a.get()), bits(a_np)) and np.array_equal(bits(b.get()), bits(b_np))
    assert a.canaries_intact() and b.canaries_intact()


def test_entries_refuse_on_the_device_too():
    from vdm4cdm_amd import hip_ops as ops
    from vdm4cdm_amd._lib import VdmError
    a, b = Vec(8, 0), Vec(8, 0)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(VdmError, match="decay"):
            ops.ema_update(a.t, b.t, bad)
    with pytest.raises(VdmError, match="same vector"):
        ops.ema_update(a.t, a.t, 0.5)
    with pytest.raises(VdmError, match="overlap"):
        ops.swap_(a.t[:6], a.t[2:])
    torch.cuda.synchronize()
    assert a.canaries_intact() and b.canaries_intact()


def test_update_and_counter_bump_replay_from_one_captured_graph():
    """update + step_inc captured once and replayed 12 times with p rewritten in between (decay 0.5: the warm-up ends at k = 8): after
    every replay the shadow is the eager sequence's and the reference's, bit for bit, and the counter ends at 12."""
    from vdm4cdm_amd import hip_ops as ops
    n, steps, decay = 4099, 12, 0.5
    rng = np.random.default_rng(5)
    ps = [rng.standard_normal(n).astype(np.float32) for _ in range(steps + 1)]
    want = R.ema_sequence(ps, decay, True)

    def run(graphed):
        shadow, p = torch.from_numpy(ps[0].copy()).to(DEV), torch.empty(n, device=DEV)
        counter = torch.zeros(1, dtype=torch.int32, device=DEV)

        def step():
            ops.ema_update(shadow, p, decay, True, counter)
            ops.step_inc(counter)

        g = None
        if graphed:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            assert counter.item() == 0 and np.array_equal(bits(shadow.cpu().numpy()), bits(ps[0]))     # capturing runs nothing
        out = []
        for i in range(steps):
            p.copy_(torch.from_numpy(ps[i + 1]))
            g.replay() if graphed else step()
            out.append(shadow.cpu().numpy())
        return out, counter.item()

    eager, k_eager = run(False)
    graph, k_graph = run(True)
    assert k_eager == k_graph == steps
    for i in range(steps):
        assert np.array_equal(bits(eager[i]), bits(want[i + 1])), f"eager update {i}"
        assert np.array_equal(bits(graph[i]), bits(want[i + 1])), f"replay {i}"
