"""k_fourier_combine forms the Legendre operands in tiles of 16 orders x RP ring pairs (hx_analysis.hip): its thread mapping, not its
arithmetic, is what these tests pin -- device-resident batches (so that k_legendre_duo and this kernel run) against the CPU oracle
at the convention of test_gpu_sht.py, max|delta| <= 1e-11 max|alm|, and bit for bit across m-chunks and ring slabs.

Sizes: lmax + 1 is no multiple of the tile (40 -> 41 orders), the polar rings have 4 .. 64 pixels (m % nphi wraps several times
inside a tile), rings are shifted and not, the equator pair has no southern partner, tasks have fewer than 4 ring blocks.
Batches: every column shape of the sweeps (16, 20, 32 columns of spin 0; 16, 20, 36, 40 of spin 2; with padding columns)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-11
SIZES = [(8, 23), (16, 40), (32, 95), (64, 100)]
NMAX = {0: 16, 2: 20}  # components of the largest batch per spin

_cache = {}


def _case(oracle, nside, lmax, spin, weighted):
    """Maps, pixel weights and the oracle's alms of the largest batch of a size: computed once, shared, never written to."""
    key = (nside, lmax, spin, weighted)
    if key not in _cache:
        rng = np.random.default_rng(1000 * nside + 10 * lmax + spin + (5 if weighted else 0))
        npix = 12 * nside**2
        maps = rng.standard_normal((NMAX[spin], npix))
        pw = 1.0 + 1e-2 * rng.standard_normal(npix) if weighted else None
        ref = oracle.map2alm(maps, nside, lmax, spin=spin, pix_weights=pw)
        for a in (maps, ref) + ((pw,) if weighted else ()):
            a.setflags(write=False)
        _cache[key] = (maps, pw, ref)
    return _cache[key]


def _resident(plan, maps, spin, pw=None):
    import torch

    dpw = None if pw is None else torch.as_tensor(pw).cuda()
    return plan.map2alm(torch.as_tensor(np.array(maps)).cuda(), spin, pix_weights=dpw).cpu().numpy()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("spin,units", [(0, 5), (0, 8), (0, 10), (0, 16), (2, 3), (2, 5), (2, 9), (2, 10)])
@pytest.mark.parametrize("nside,lmax", SIZES)
def test_resident_batches_match_the_oracle(oracle, nside, lmax, spin, units, weighted):
    import heracles_amd as hx

    maps, pw, ref = _case(oracle, nside, lmax, spin, weighted)
    ncomp = units * (2 if spin else 1)
    got = _resident(hx.get_plan(nside, lmax), maps[:ncomp], spin, pw)
    want = ref[:ncomp]
    assert got.shape == want.shape
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"nside {nside} lmax {lmax} spin {spin} units {units} weighted {weighted}: max err {err:.3e}, scale {scale:.3e}")
    assert err <= TOL * scale


@pytest.mark.parametrize("spin,ncomp", [(2, 20), (0, 10)])
def test_m_chunks_do_not_change_a_bit(spin, ncomp):
    """Ten fields (and ten maps) at (64, 191) cut into m-chunks.  A chunk holds at least one order whatever the budget: a budget of one
    byte gives 192 chunks of one order, which start at every m; 5e5 bytes give chunks of a few orders (an order takes 82 KB of
    operands and up to 74 KB of rows), more than 192 / 16 = 12 of them, so that some start at an m that is no multiple of the tile;
    1.5e6 and 4e6 bytes fewer and longer ones, with tile boundaries inside a chunk that begins in the middle of a tile."""
    import heracles_amd as hx

    nside, lmax = 64, 191
    rng = np.random.default_rng(64191 + spin)
    maps = rng.standard_normal((ncomp, 12 * nside**2))
    plan = hx.get_plan(nside, lmax)
    whole = _resident(plan, maps, spin)
    assert plan.last_chunks == 1
    for budget, least in ((1.0, 192), (5e5, 13), (1.5e6, 4), (4e6, 3)):
        hx._lib.set_scratch_budget(budget)
        try:
            cut = _resident(plan, maps, spin)
            nchunk = plan.last_chunks
        finally:
            hx._lib.set_scratch_budget(0)
        print(f"spin {spin}: budget {budget:g} -> {nchunk} chunks")
        assert nchunk >= least, (budget, nchunk)
        np.testing.assert_array_equal(cut, whole)


def test_host_maps_streamed_in_slabs_equal_resident_maps():
    """The StreamSweep launch (tile0 != 0: the operand rows of one slab of rings at a time) gives the bits of the resident sweep."""
    import heracles_amd as hx

    nside, lmax = 64, 128
    rng = np.random.default_rng(64128)
    npix = 12 * nside**2
    plan = hx.get_plan(nside, lmax)
    pw = 1.0 + 1e-2 * rng.standard_normal(npix)
    for spin, ncomp in ((2, 20), (0, 10), (0, 16), (2, 10)):
        m = rng.standard_normal((ncomp, npix))
        ref = _resident(plan, m, spin, pw)
        got = plan.map2alm(m, spin, pix_weights=pw)
        np.testing.assert_array_equal(np.asarray(got), ref)
