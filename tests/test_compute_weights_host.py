"""Host-side logic of ``compute_pixel_weights``: argument checks, the cache and its key, the export.  No GPU: the solve itself is
pinned in tests/test_gpu_compute_weights.py."""

import warnings

import numpy as np
import pytest


def test_exported():
    import heracles_amd
    from heracles_amd import weights

    assert "compute_pixel_weights" in heracles_amd.__all__
    assert heracles_amd.compute_pixel_weights is weights.compute_pixel_weights
    assert "hx_pixel_weights_solve" in heracles_amd._lib.SYMBOLS


@pytest.mark.parametrize("nside,lmax", [(8, 13), (6, 10), (16, 48), (1, 2)])
def test_band_limit_beyond_three_halves_nside_is_refused(nside, lmax):
    """Past lmax = 3 nside / 2 the weights make the quadrature worse than unit weights (nside 8, lmax 13: 5.7e-2 against 6.0e-3):
    refused before anything touches the GPU, with a message that says why."""
    from heracles_amd import weights

    with pytest.raises(ValueError, match="3 nside / 2"):
        weights.compute_pixel_weights(nside, lmax)
    with pytest.raises(ValueError, match="worse"):
        weights.compute_pixel_weights(nside, lmax, device="cuda", compressed=True, info=True)


def test_other_bad_arguments():
    from heracles_amd import weights

    for kw in (dict(nside=0), dict(nside=8, lmax=-1), dict(nside=8, epsilon=-1e-3), dict(nside=8, epsilon=float("nan")), dict(nside=8, itmax=-1)):
        with pytest.raises(ValueError):
            weights.compute_pixel_weights(**kw)


def test_cache_key():
    from heracles_amd import weights

    key = weights._solve_key(8, None, 1e-12, None, None)
    assert key == (8, 12, 1e-12, weights.DEFAULT_ITMAX, None)
    assert weights._solve_key(np.int64(8), 12, 1e-12, weights.DEFAULT_ITMAX, None) == key  # the defaults spelled out: the same entry
    others = [weights._solve_key(8, 11, 1e-12, None, None), weights._solve_key(8, None, 1e-9, None, None), weights._solve_key(8, None, 1e-12, 7, None),
              weights._solve_key(8, None, 1e-12, None, "cuda"), weights._solve_key(16, None, 1e-12, None, None)]
    assert len({key, *others}) == 6
    import torch

    assert weights._solve_key(8, None, 1e-12, None, torch.device("cuda")) == weights._solve_key(8, None, 1e-12, None, "cuda")
    assert hash(key) == hash(weights._solve_key(8, None, 1e-12, None, None))


def test_cached_results_are_served_and_released():
    """A cached entry is returned without a solve (none is possible here), as copies the caller may change; an entry that stopped
    short of epsilon warns every time it is handed out; release_caches() drops the entries."""
    import heracles_amd
    from heracles_amd import weights

    nside = 4
    x = np.linspace(-1e-2, 1e-2, weights.compressed_size(nside))
    full = 1.0 + np.arange(12 * nside**2, dtype=float)
    stats = {"iterations": 9, "rel_gradient": 5e-13, "max_residual": 1e-15}
    weights._computed[weights._solve_key(nside, None, 1e-12, None, None)] = (x, full, stats)
    weights._computed[weights._solve_key(nside, None, 1e-12, 3, None)] = (x, full, {"iterations": 3, "rel_gradient": 1e-4, "max_residual": 1e-6})
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            w = weights.compute_pixel_weights(nside)
            c, info = weights.compute_pixel_weights(nside, 6, compressed=True, info=True)
        np.testing.assert_array_equal(w, full)
        np.testing.assert_array_equal(c, x)
        assert info == stats
        w[0] = -1.0
        c[0] = -1.0
        info["iterations"] = 0
        assert weights.compute_pixel_weights(nside)[0] == 1.0 and weights.compute_pixel_weights(nside, compressed=True)[0] == x[0]
        assert weights.compute_pixel_weights(nside, info=True)[1]["iterations"] == 9
        with pytest.warns(RuntimeWarning, match="epsilon = 1e-12 was not reached in 3 iterations"):
            weights.compute_pixel_weights(nside, itmax=3)
    finally:
        heracles_amd.release_caches()
    assert not weights._computed


def test_mapper_accepts_the_mode_and_no_other_string():
    import heracles_amd

    m = heracles_amd.HipHealpixMapper(8, 12, pixel_weights="compute")
    assert m.pixel_weights == "compute"  # nothing is computed before the first transform
    with pytest.raises(ValueError, match="compute"):
        heracles_amd.HipHealpixMapper(8, 12, pixel_weights="full")._load_weights()
    with pytest.raises(ValueError, match="3 nside / 2"):
        heracles_amd.HipHealpixMapper(8, 13, pixel_weights="compute")._load_weights()
