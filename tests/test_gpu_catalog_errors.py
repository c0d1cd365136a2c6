"""The error readout of the catalogue contexts on the MI355X: the NaN counters of every (field, column) and the invalid-position counter
of every (resolution, lon, lat) group, read back through hx_catmap_moments, hx_catalm_moments and hx_catmap_moments_sel.  Each catalogue
has three fields in TWO groups, so that the counter of the second group, the NaN slots of the second field and, for the views, the
counters of the second selection are all read from offsets other than zero."""

import warnings

import numpy as np
import pytest

import heracles_amd as hx

pytestmark = pytest.mark.gpu

N = 2000


def _columns():
    rng = np.random.default_rng(23)
    return {
        "lon": rng.uniform(0, 360, N),
        "lat": np.degrees(np.arcsin(rng.uniform(-1, 1, N))),
        "lon2": rng.uniform(0, 360, N),
        "lat2": np.degrees(np.arcsin(rng.uniform(-1, 1, N))),
        "g1": rng.normal(0, 0.3, N),
        "g2": rng.normal(0, 0.3, N),
        "w": rng.choice([0.0, 0.5, 1.0, 2.0], N, p=[0.1, 0.2, 0.5, 0.2]),
        "bin": (np.arange(N) % 2).astype(np.float64),
    }


def _fields(first, second):
    """Positions and weights on (lon, lat) with the mapper ``first``, shear on (lon2, lat2) with ``second``: groups 0 and 1."""
    return {
        "POS": hx.Positions(first, "lon", "lat", overdensity=False),
        "SHE": hx.Shears(second, "lon2", "lat2", "g1", "g2", "w"),
        "WHT": hx.Weights(first, "lon", "lat", "w"),
    }


def _healpix():
    return _fields(hx.HipHealpixMapper(8, 16, deconvolve=False), hx.HipHealpixMapper(16, 32, deconvolve=False))


def _discrete():
    return _fields(hx.HipDiscreteMapper(16), hx.HipDiscreteMapper(32))


def _kept(cols, count, where=None):
    """The first ``count`` rows with a non-zero weight (and ``where``)."""
    ok = cols["w"] != 0 if where is None else (cols["w"] != 0) & where
    return np.flatnonzero(ok)[:count]


def _run(call, fields, cols, page_size=700):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return call(fields, {0: hx.ArrayCatalog(cols, page_size=page_size)})


CASES = [(hx.map_catalogs, _healpix), (hx.catalog_alms, _discrete)]
IDS = ["map_catalogs", "catalog_alms"]


@pytest.mark.parametrize("call,fields", CASES, ids=IDS)
def test_bad_positions_of_the_second_group(call, fields):
    cols = _columns()
    cols["lat2"][_kept(cols, 3)] = 91.0
    with pytest.raises(ValueError, match="3 positions of field 'SHE'"):
        _run(call, fields(), cols)


@pytest.mark.parametrize("call,fields", CASES, ids=IDS)
def test_bad_positions_of_the_first_group(call, fields):
    cols = _columns()
    cols["lat"][_kept(cols, 3)] = 91.0
    with pytest.raises(ValueError, match="3 positions of field 'POS'"):
        _run(call, fields(), cols)


@pytest.mark.parametrize("call,fields", CASES, ids=IDS)
def test_nan_in_the_imaginary_column(call, fields):
    cols = _columns()
    cols["g2"][_kept(cols, 2)] = np.nan
    with pytest.raises(ValueError, match='invalid values in column "g2"'):
        _run(call, fields(), cols)


def test_nan_on_a_row_of_weight_zero_is_no_error():
    cols = _columns()
    clean = _run(hx.map_catalogs, _healpix(), cols)
    row = np.flatnonzero(cols["w"] == 0)[0]
    cols["g1"][row] = np.nan
    got = _run(hx.map_catalogs, _healpix(), cols)
    assert list(got) == list(clean) == [("POS", 0), ("SHE", 0), ("WHT", 0)]
    for key, m in got.items():
        np.testing.assert_array_equal(np.asarray(m), np.asarray(clean[key]), err_msg=str(key))


def test_views_report_only_their_own_bad_positions():
    """Two views in one pass, two groups: three invalid positions of the second group in the rows of the second view.  The first view
    is mapped (its maps are in ``out`` when the second raises) and the second reports exactly its three."""
    cols = _columns()
    cols["lat2"][_kept(cols, 3, cols["bin"] == 1)] = 91.0
    base = hx.ArrayCatalog(cols, page_size=700)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="3 positions of field 'SHE'"):
            hx.map_catalogs(_healpix(), {"a": base["bin==0"], "b": base["bin==1"]}, out=out)
    assert list(out) == [("POS", "a"), ("SHE", "a"), ("WHT", "a")]
