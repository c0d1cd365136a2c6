"""hx_reorder, hx_ud_grade and read_vmap of a NESTED file at production nside against RING <-> NEST built from the projection of the
pixel centre (tests/pixel_reference.py: integers only, no index formula or square root shared with the kernels)."""

import numpy as np
import pytest

import pixel_reference as pr

pytestmark = pytest.mark.gpu

UNSEEN = -1.6375e30


def _reorder(nside, to_ring, src):
    import torch

    import heracles_amd as hx

    out = torch.empty_like(src)
    hx._lib.check(hx._lib.load().hx_reorder(nside, to_ring, 1, hx._lib.ptr(src), hx._lib.ptr(out)))
    return out


@pytest.mark.parametrize("nside", [1, 2, 4, 32, 256, 4096, 8192])
def test_reorder_is_the_exact_permutation(nside):
    """A device map whose value at pixel p is p (exact in float64), both directions; every pixel up to nside 256, above that every
    ring's first and last pixel, the cap boundaries, the face corners and 10^6 random pixels."""
    import torch

    npix = 12 * nside**2
    src = torch.arange(npix, dtype=torch.float64, device="cuda")
    pos = np.arange(npix) if nside <= 256 else pr.sample_pixels(nside, np.random.default_rng(nside), 1_000_000)
    dpos = torch.as_tensor(pos, device="cuda")
    for to_ring, exact in ((1, pr.ring2nest_exact), (0, pr.nest2ring_exact)):  # out[p] = in[other index of p]
        out = _reorder(nside, to_ring, src)
        got = out[dpos].cpu().numpy().astype(np.int64)
        del out
        np.testing.assert_array_equal(got, exact(nside, pos), err_msg=f"nside {nside}, to_ring={to_ring}")


def _input_map(nside, seed):
    """Non-integer values over ten decades, on the device."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    npix = 12 * nside**2
    m = torch.rand(npix, dtype=torch.float64, device="cuda", generator=g) * 2.0 - 1.0
    m *= 10.0 ** (torch.rand(npix, dtype=torch.float64, device="cuda", generator=g) * 10.0 - 5.0)
    return m


def _expected_degrade(rows):
    """oracle.ud_grade's arithmetic on the children of each parent, a C-contiguous (n, rat2) array in NEST order."""
    rows = np.ascontiguousarray(rows)
    with np.errstate(invalid="ignore"):
        goods = ~((np.absolute(rows - UNSEEN) <= 1e-15 + 1e-5 * np.absolute(UNSEEN)) | (~np.isfinite(rows)))
        out = np.sum(rows * goods, axis=1)
        nhit = goods.sum(axis=1)
        out[nhit != 0] = out[nhit != 0] / nhit[nhit != 0]
    out[nhit == 0] = UNSEEN
    return out


@pytest.fixture(scope="module")
def map4096():
    import torch

    m = _input_map(4096, 4096)
    yield m
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nside_out", [2048, 1024, 256, 16])
def test_degrade_from_4096_on_sampled_parents(map4096, nside_out):
    """4, 16, 256 and 65 536 children: the three branches of numpy's pairwise sum and a deep split.  UNSEEN, NaN and +-inf are planted
    in children of sampled parents and of their NEST neighbours, one sampled parent is unseen throughout; the expected values come from
    the children gathered through the exact inverse map, bit for bit.  (2^22 / rat2 parents at most: 64 for 65 536 children.)"""
    import torch

    from heracles_amd.mapper import ud_grade

    nside_in = 4096
    rat2 = (nside_in // nside_out) ** 2
    rng = np.random.default_rng(nside_out)
    nsample = min(2000, 2**22 // rat2)
    pout = pr.sample_pixels(nside_out, rng, nsample)
    pout = np.unique(np.concatenate([pout[:: max(1, pout.size // nsample)], pout[-1:]]))
    parents = pr.ring2nest_exact(nside_out, pout)
    src = map4096.clone()
    # plant: one special value in a random child of the first parents and of their neighbours; every child of one parent
    npix_out = 12 * nside_out**2
    plant = np.unique(np.concatenate([parents[:24], (parents[:24] + 1) % npix_out, (parents[:24] - 1) % npix_out]))
    special = np.resize(np.array([UNSEEN, np.nan, np.inf, -np.inf, UNSEEN * (1 + 5e-6), 0.0]), plant.size)
    child = pr.nest2ring_exact(nside_in, plant * rat2 + rng.integers(0, rat2, plant.size))
    src[torch.as_tensor(child, device="cuda")] = torch.as_tensor(special, device="cuda")
    src[torch.as_tensor(pr.nest2ring_exact(nside_in, parents[30] * rat2 + np.arange(rat2)), device="cuda")] = UNSEEN
    got = ud_grade(src, nside_out)
    assert got.shape == (npix_out,)
    children = pr.nest2ring_exact(nside_in, (parents[:, None] * rat2 + np.arange(rat2)[None, :]).ravel())
    rows = src[torch.as_tensor(children, device="cuda")].cpu().numpy().reshape(parents.size, rat2)
    want = _expected_degrade(rows)
    have = got[torch.as_tensor(pout, device="cuda")].cpu().numpy()
    assert want[30] == UNSEEN and np.isnan(want).any()
    np.testing.assert_array_equal(have, want)


def test_degrade_by_256_matches_the_oracle_on_the_whole_map(oracle):
    """65 536 children per parent at a size the oracle handles in full (nside 256 -> 1): numpy sums such a row in pieces of 8192."""
    from heracles_amd.mapper import ud_grade

    m = _input_map(256, 256).cpu().numpy()
    m[::1001] = UNSEEN
    np.testing.assert_array_equal(ud_grade(m, 1), oracle.ud_grade(m, 1))


def test_upgrade_1024_to_4096_on_sampled_pixels():
    import torch

    from heracles_amd.mapper import ud_grade

    src = _input_map(1024, 1024)
    got = ud_grade(src, 4096)
    pout = pr.sample_pixels(4096, np.random.default_rng(7), 2000)
    parent = pr.nest2ring_exact(1024, pr.ring2nest_exact(4096, pout) >> 4)
    np.testing.assert_array_equal(got[torch.as_tensor(pout, device="cuda")].cpu().numpy(),
                                  src[torch.as_tensor(parent, device="cuda")].cpu().numpy())


def test_read_vmap_of_a_nested_file_at_nside_1024(tmp_path):
    """The RING map read from a NESTED file == the exact permutation of what was written (unseen pixels zero)."""
    import heracles_amd as hx
    from test_gpu_widen import _write_healpix_table

    nside = 1024
    npix = 12 * nside**2
    rng = np.random.default_rng(1024)
    nested = np.arange(npix) + 0.25
    nested[rng.choice(npix, 500, replace=False)] = UNSEEN
    path = tmp_path / "nested.fits"
    _write_healpix_table(path, [nested], nside, ordering="NESTED")
    got = hx.read_vmap(path)
    want = nested[pr.ring2nest_exact(nside, np.arange(npix))]
    want[want == UNSEEN] = 0.0
    np.testing.assert_array_equal(got, want)
