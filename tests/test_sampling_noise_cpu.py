"""sampling.ChainNoise against the keying rules of the samplers, written out literally: which generator, seeded how, draws z_1 and
draw d of a chain, in the ancestral and the DDNM index convention, and what the device loops are handed (checked on device="cpu")."""
import pytest
import torch

from vdm4cdm_amd.sampling import ChainNoise

B, CUBE = 3, (1, 4, 4, 4)
SHAPE = (B,) + CUBE
SEEDS = [7, 9, 7]


def _noise(who="sample", batch=B, **kw):
    return ChainNoise(who, batch, CUBE, "cpu", **kw)


def _fields(n):
    g = torch.Generator().manual_seed(123)
    return [torch.randn(SHAPE, generator=g) for _ in range(n)]


# ------------------------------------------------------------------------------ seed: one stream for the batch
@pytest.mark.parametrize("ddnm", [False, True], ids=["ancestral", "ddnm"])
def test_seed_keys_one_generator_for_z1_and_one_for_the_draws(ddnm):
    noise = _noise(seed=5, z1_in_noises=ddnm)
    z = noise.z1()
    assert z.dtype == torch.float32 and z.is_contiguous()
    assert torch.equal(z, torch.randn(SHAPE, generator=torch.Generator().manual_seed(5)))
    g = torch.Generator().manual_seed(6)
    for d in range(3):
        assert torch.equal(noise.host_draw(d, z), torch.randn(SHAPE, generator=g)), d
    assert noise.keyed


# ------------------------------------------------------------------------------ seeds: one chain per row
@pytest.mark.parametrize("ddnm", [False, True], ids=["ancestral", "ddnm"])
def test_seeds_key_every_row_as_the_batch_1_chain_of_its_seed(ddnm):
    noise = _noise(seeds=SEEDS, z1_in_noises=ddnm)
    z = noise.z1()
    draws = [noise.host_draw(d, z) for d in range(3)]
    assert z.shape == SHAPE and all(e.shape == SHAPE for e in draws)
    for r, s in enumerate(SEEDS):
        assert torch.equal(z[r:r + 1], torch.randn((1,) + CUBE, generator=torch.Generator().manual_seed(s))), r
        g = torch.Generator().manual_seed(s + 1)
        one = _noise(batch=1, seed=s, z1_in_noises=ddnm)
        z_one = one.z1()
        assert torch.equal(z[r:r + 1], z_one), r
        for d in range(3):
            assert torch.equal(draws[d][r:r + 1], torch.randn((1,) + CUBE, generator=g)), (r, d)
            assert torch.equal(draws[d][r:r + 1], one.host_draw(d, z_one)), (r, d)
    assert torch.equal(z[0], z[2]) and not torch.equal(z[0], z[1])
    for e in draws:
        assert torch.equal(e[0], e[2]) and not torch.equal(e[0], e[1])


def test_seeds_with_a_supplied_z_key_the_step_noise_only():
    z_in = torch.randn(SHAPE, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    noise = _noise(seeds=SEEDS)
    z = noise.z1(z_in)
    assert z.dtype == torch.float32 and torch.equal(z, z_in.float()) and z.data_ptr() != z_in.data_ptr()
    f32 = z_in.float()
    assert _noise(seeds=SEEDS).z1(f32).data_ptr() != f32.data_ptr()                  # cloned even when nothing is converted
    g = torch.Generator().manual_seed(SEEDS[1] + 1)
    assert torch.equal(noise.host_draw(0, z)[1:2], torch.randn((1,) + CUBE, generator=g))


# ------------------------------------------------------------------------------ noises: the fields themselves
def test_noises_in_the_ancestral_convention():
    fields = _fields(4)
    noise = _noise(noises=fields, seed=5)                    # (seed= may accompany noises= here: it keys z_1)
    z = noise.z1()
    assert torch.equal(z, torch.randn(SHAPE, generator=torch.Generator().manual_seed(5)))
    for i in range(4):
        assert torch.equal(noise.host_draw(i, z), fields[i]), i
    assert torch.equal(noise.host_draw(1, z.double()), fields[1].double())          # cast to the chain's dtype
    noise.prime()
    assert torch.equal(noise.feed.buf, fields[0])
    for i in (2, 0, 3):
        noise.load(i)
        assert torch.equal(noise.feed.buf, fields[i]), i
    _noise(noises=fields[:1])                                # no length is asked of the ancestral list


def test_noises_in_the_ddnm_convention():
    n_draws = 4
    fields = _fields(1 + n_draws)
    noise = _noise("get_ddnm_result", noises=fields, n_fields=1 + n_draws, z1_in_noises=True)
    z = noise.z1()
    assert torch.equal(z, fields[0]) and z.data_ptr() != fields[0].data_ptr()
    for d in range(n_draws):
        assert torch.equal(noise.host_draw(d, z), fields[d + 1]), d
    noise.prime()
    assert torch.equal(noise.feed.buf, fields[1])            # draw 0
    for d in (3, 1, 0):
        noise.load(d)
        assert torch.equal(noise.feed.buf, fields[d + 1]), d
    for n in (n_draws, 2 + n_draws):
        with pytest.raises(ValueError) as e:
            _noise("get_ddnm_result", noises=(fields + fields)[:n], n_fields=1 + n_draws, z1_in_noises=True)
        assert str(e.value) == f"get_ddnm_result: {n} noises, the schedule draws {1 + n_draws} fields (z_1 first)"


def test_noise_feed_blocks_cover_every_index():
    """The block upload of the feed at a block size below the list's length: every field arrives, in any order of loads."""
    fields = _fields(5)
    noise = _noise(noises=fields)
    noise.z1()
    noise.feed.blk = 2
    for i in (0, 1, 2, 4, 3, 0):
        noise.load(i)
        assert torch.equal(noise.feed.buf, fields[i]), i


# ------------------------------------------------------------------------------ unkeyed
@pytest.mark.parametrize("ddnm", [False, True], ids=["ancestral", "ddnm"])
def test_unkeyed_chain_draws_z1_from_the_global_rng_and_leaves_the_steps_to_the_loop(ddnm):
    noise = _noise(z1_in_noises=ddnm)
    torch.manual_seed(3)
    z = noise.z1()
    torch.manual_seed(3)
    assert torch.equal(z, torch.randn(SHAPE))
    state = torch.get_rng_state()
    assert not noise.keyed and noise.host_draw(0, z) is None
    assert torch.equal(torch.get_rng_state(), state)


# ------------------------------------------------------------------------------ device form
@pytest.mark.parametrize("ddnm", [False, True], ids=["ancestral", "ddnm"])
def test_device_form(ddnm):
    big = (1 << 40) + 5
    noise = _noise(seeds=[7, big, 7], z1_in_noises=ddnm)
    assert noise.seeds_dev.dtype == torch.int64 and noise.seeds_dev.tolist() == [7, big, 7] and not noise.batch_stream
    assert noise.feed is None

    noise = _noise(seed=5, z1_in_noises=ddnm)
    state = torch.get_rng_state()
    assert noise.seeds_dev.dtype == torch.int64 and noise.seeds_dev.tolist() == [5] and noise.batch_seed == 5 and noise.batch_stream
    assert torch.equal(torch.get_rng_state(), state)         # a given seed: nothing is drawn

    noise = _noise(z1_in_noises=ddnm)                        # none given: one random 62-bit seed, drawn once, at the first use (after z_1)
    noise.z1()
    torch.manual_seed(11)
    state = torch.get_rng_state()
    got = noise.seeds_dev.tolist()
    after = torch.get_rng_state()
    torch.manual_seed(11)
    expect = int(torch.randint(0, 2 ** 62, (1,)).item())
    assert got == [expect] and noise.batch_seed == expect and noise.batch_stream
    assert torch.equal(torch.get_rng_state(), after) and not torch.equal(after, state)       # exactly that one draw
    assert noise.seeds_dev.tolist() == [expect] and torch.equal(torch.get_rng_state(), after)
    assert not noise.keyed                                   # the torch backend's chain stays unkeyed

    noise = _noise(noises=_fields(2), z1_in_noises=ddnm, n_fields=2 if ddnm else None)
    state = torch.get_rng_state()
    assert noise.seeds_dev is None and not noise.batch_stream
    assert torch.equal(torch.get_rng_state(), state)
    noise.z1()
    assert noise.feed.buf.shape == SHAPE and noise.feed.buf.dtype == torch.float32


# ------------------------------------------------------------------------------ errors
def _message(**kw):
    with pytest.raises(ValueError) as e:
        _noise(**kw)
    return str(e.value)


def test_errors_of_sample():
    f = _fields(2)
    assert _message(seeds=[1, 2]) == "sample: 2 seeds for batch_size=3 (one seed per chain)"
    assert _message(seeds=[1, 2], seed=1) == "sample: 2 seeds for batch_size=3 (one seed per chain)"      # the count is checked first
    assert _message(seeds=SEEDS, seed=1) == "sample: seeds= cannot be combined with seed= or noises="
    assert _message(seeds=SEEDS, noises=f) == "sample: seeds= cannot be combined with seed= or noises="
    assert _message(seeds=SEEDS, seed=1, noises=f) == "sample: seeds= cannot be combined with seed= or noises="


def test_errors_of_get_ddnm_result():
    f = _fields(3)
    kw = dict(who="get_ddnm_result", z1_in_noises=True, n_fields=3)
    combined = "get_ddnm_result: seed=, seeds= and noises= cannot be combined"
    assert _message(seeds=[1, 2], **kw) == "get_ddnm_result: 2 seeds for 3 rows of y (one seed per chain)"
    assert _message(seeds=[1, 2], seed=1, **kw) == "get_ddnm_result: 2 seeds for 3 rows of y (one seed per chain)"
    assert _message(seeds=SEEDS, seed=1, **kw) == combined
    assert _message(seeds=SEEDS, noises=f, **kw) == combined
    assert _message(seed=1, noises=f, **kw) == combined
    assert _message(seed=1, noises=f[:2], **kw) == combined                          # combination before the count of fields
    assert _message(noises=f[:2], **kw) == "get_ddnm_result: 2 noises, the schedule draws 3 fields (z_1 first)"
