"""Kernel-level tests of conditioning dropout (ABI v21 additions): vdm_cond_keep against the Philox reference (tests/_cfg_ref.py),
vdm_mask_rows as a select, and the fused head with a per-row keep (vdm_diffuse_pack_fields_keep) against vdm_diffuse_pack_fields on a
conditioning whose dropped rows the host zeroed.  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from _cfg_ref import keep_rows
from helpers import grf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20240611
bits = lambda t: t.contiguous().view(torch.uint8)


# ------------------------------------------------------------------------------------------ vdm_cond_keep
@pytest.mark.parametrize("step", [None, 0, 5])
@pytest.mark.parametrize("row0", [0, 2 ** 32 + 5])
def test_cond_keep_equals_the_philox_reference(row0, step):
    from vdm4cdm_amd import hip_ops as ops
    try:
        if step is not None:
            ops.SEED_STEP = torch.full((1,), step, dtype=torch.int32, device=DEV)
        for rows in (1, 3, 64, 257, 4096):
            for p in (0.0, 0.1, 0.5, 1.0):
                got = ops.cond_keep(p, SEED, rows, DEV, row0=row0).cpu().numpy()
                ref = keep_rows(SEED, p, row0, rows, step=step)
                assert got.dtype == np.float32 and np.array_equal(got, ref), (rows, p, np.flatnonzero(got != ref)[:8])
                if p == 0.0:
                    assert got.all()
                if p == 1.0:
                    assert not got.any()
    finally:
        ops.SEED_STEP = None


# ------------------------------------------------------------------------------------------ vdm_mask_rows
@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("dim", [6, 64, 4 * 16 ** 3], ids=["scalar6", "vec64", "vec4x16cube"])
def test_mask_rows_is_a_select(dim, inplace):
    """keep (1, 0, 1): kept rows bit-equal (a -0 and a NaN in them included), the dropped row +0 although NaN / Inf / -0 sit in it."""
    from vdm4cdm_amd import hip_ops as ops
    g = torch.Generator().manual_seed(dim)
    v = torch.randn(3, dim, generator=g)
    v[0, 1], v[2, 0] = -0.0, float("nan")
    v[1, 0], v[1, 1], v[1, 2], v[1, dim - 1] = float("nan"), float("inf"), -0.0, float("-inf")
    keep = torch.tensor([1.0, 0.0, 1.0], device=DEV)
    src = v.to(DEV)
    out = ops.mask_rows(src, keep, out=src if inplace else None)
    assert (out.data_ptr() == src.data_ptr()) == inplace
    out = out.cpu()
    assert torch.equal(bits(out[0]), bits(v[0])) and torch.equal(bits(out[2]), bits(v[2]))
    assert torch.equal(bits(out[1]), bits(torch.zeros(dim)))                 # +0: every byte zero
    if not inplace:
        assert torch.equal(bits(src.cpu()), bits(v))


def test_mask_rows_scalar_path_on_an_unaligned_view():
    """dim % 4 == 0 but the pointer is 4 bytes off a 16-byte boundary: the scalar path, same result."""
    from vdm4cdm_amd import hip_ops as ops
    buf = torch.arange(1 + 3 * 8, dtype=torch.float32, device=DEV) + 1.0
    v = buf[1:].view(3, 8)
    assert v.data_ptr() % 16 == 4
    out = ops.mask_rows(v, torch.tensor([0.0, 1.0, 0.0], device=DEV))
    assert torch.equal(out.cpu(), torch.tensor([0.0, 1.0, 0.0]).view(3, 1) * v.cpu())


# ------------------------------------------------------------------------------------------ vdm_diffuse_pack_fields_keep
PER_ONE_BLOCK = 4 ** 3                      # a sample fits one workgroup
PER_TWO_BLOCKS = 4 * (256 * 16 + 1)         # the smallest per with blocks_per_n > 1: per / 4 float4 groups > 256 threads x 16


@pytest.mark.parametrize("drawn", [False, True], ids=["eps_supplied", "eps_drawn"])
@pytest.mark.parametrize("per", [PER_ONE_BLOCK, PER_TWO_BLOCKS], ids=["one_block", "two_blocks"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_head_with_keep_equals_the_head_on_host_zeroed_conditioning(k, dtype, per, drawn):
    from vdm4cdm_amd import hip_ops as ops
    n = 3
    g = torch.Generator().manual_seed(7 * k + per % 11)
    x = torch.randn(n, 1, 1, per, generator=g).to(DEV)
    cond = torch.randn(n, k, 1, 1, per, generator=g).to(DEV)
    eps = None if drawn else torch.randn(n, 1, 1, per, generator=g).to(DEV)
    al, si = torch.tensor([0.9, 0.5, 0.1], device=DEV), torch.tensor([0.3, 0.8, 0.99], device=DEV)
    keep = torch.tensor([1.0, 0.0, 1.0], device=DEV)
    kw = dict(eps=eps, seed=123456789012345, stream_id=7, want_z=True)
    zeroed = cond.clone()
    zeroed[1] = 0.0
    z_ref, p_ref = ops.diffuse_pack_fields(x, zeroed, al, si, dtype, **kw)
    z_all, p_all = ops.diffuse_pack_fields(x, cond, al, si, dtype, **kw)
    assert not torch.equal(bits(p_ref), bits(p_all)), "zeroing row 1 changes nothing: the check would be vacuous"

    def same(zp, ref, what):
        assert torch.equal(bits(zp[0]), bits(ref[0])), f"{what}: z_t differs"
        bad = (bits(zp[1]) != bits(ref[1])).flatten().nonzero().flatten()
        assert bad.numel() == 0, f"{what}: {bad.numel()} bytes of packed differ, first at {bad[:8].tolist()}"
    same(ops.diffuse_pack_fields(x, cond, al, si, dtype, keep_s=keep, **kw), (z_ref, p_ref), "keep (1, 0, 1)")
    poisoned = cond.clone()
    poisoned[1] = float("nan")                                              # the dropped row's planes are not read into the output
    same(ops.diffuse_pack_fields(x, poisoned, al, si, dtype, keep_s=keep, **kw), (z_ref, p_ref), "NaN in the dropped row")
    same(ops.diffuse_pack_fields(x, cond, al, si, dtype, keep_s=torch.ones(n, device=DEV), **kw), (z_all, p_all), "keep all ones")
    same(ops.diffuse_pack_fields(x, cond, al, si, dtype, keep_s=None, **kw), (z_all, p_all), "keep_s = NULL")
    if k == 1:                                                              # the bits of vdm_diffuse_pack, with and without the keep
        same(ops.diffuse_pack(x, zeroed[:, 0], al, si, dtype, **kw), (z_ref, p_ref), "vdm_diffuse_pack")
        same(ops.diffuse_pack(x, poisoned[:, 0], al, si, dtype, keep_s=keep, **kw), (z_ref, p_ref), "diffuse_pack(keep_s=)")
