"""The catalogue the order-exact tests at production key widths share (test_gpu_mapper.py, test_gpu_fields.py, test_gpu_selections.py),
and the sequential reference they compare with.

K = 3000 sky positions (two of them the poles), n = 200 003 rows each at one of them, a fifth of the rows at ONE position, shuffled so
that a pixel's rows interleave with all the others; values spread over 16 decades, so that a sum depends on its order.  The reference is
``np.add.at`` in catalogue order on compact indices (np.unique): the touched pixels only, no full-size host map."""

import numpy as np

K, N = 3000, 200_003
MIN_TOUCHED = 2000


def values(rng, shape):
    return rng.standard_normal(shape) * 10.0 ** rng.integers(-8, 8, shape)


def rows(seed):
    """(rng, lon[N], lat[N]) in degrees."""
    rng = np.random.default_rng(seed)
    lon_k = rng.uniform(0.0, 360.0, K)
    lat_k = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, K)))
    lat_k[0], lat_k[1] = 90.0, -90.0
    which = rng.integers(0, K, N)
    which[: N // 5] = 2  # the crowded position
    rng.shuffle(which)
    return rng, lon_k[which], lat_k[which]


def sequential(ipix, vals, fill=0.0, reverse=False):
    """vals [nrow][n] added in catalogue order (or the reverse) to maps that start at `fill`: (touched pixels, sums [nrow][touched])."""
    vals = np.atleast_2d(vals)
    upix, inv = np.unique(ipix, return_inverse=True)
    inv = inv.reshape(-1)
    out = np.full((vals.shape[0], upix.size), fill)
    step = -1 if reverse else 1
    for r in range(vals.shape[0]):
        np.add.at(out[r], inv[::step], vals[r][::step])
    return upix, out


def reference(ipix, vals, fill=0.0):
    """The sequential sums, after asserting that these inputs can tell a wrong order: at least MIN_TOUCHED pixels, and in every value
    row at least half of them change when the same rows are added in reversed order."""
    upix, fwd = sequential(ipix, vals, fill)
    _, rev = sequential(ipix, vals, fill, reverse=True)
    assert upix.size >= MIN_TOUCHED, upix.size
    changed = (fwd != rev).mean(axis=1)
    assert (changed >= 0.5).all(), changed
    return upix, fwd


def check_maps(maps, upix, want, fill, where=""):
    """maps: device tensor [nrow][npix] (or [npix]).  Exact equality at the touched pixels; every other pixel still holds `fill`
    (the entries that differ from it are counted on the device)."""
    import torch

    maps = maps.reshape(-1, maps.shape[-1])
    want = np.atleast_2d(want)
    assert maps.shape[0] == want.shape[0], (maps.shape, want.shape)
    got = maps[:, torch.as_tensor(upix, device=maps.device)].cpu().numpy()
    np.testing.assert_array_equal(got, want, err_msg=where)
    differ = (maps != fill).sum(dim=1).cpu().numpy()
    np.testing.assert_array_equal(differ, (want != fill).sum(axis=1), err_msg=where + " (pixels that differ from the initial value)")
