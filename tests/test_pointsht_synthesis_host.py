"""HipDiscreteMapper.sample without a device: coordinate conversion, choice of accuracy and shape handling, with get_point_sht
replaced by a numpy stand-in that records what it is asked for.  (That the new entry points are declared, bound and given argtypes is
tests/test_cabi.py's comparison of include/hxsht.h with _lib.SYMBOLS.)"""
import numpy as np
import pytest

import heracles_amd.discrete as discrete
from heracles_amd import HipDiscreteMapper


class _Recorder:
    """Stands in for PointSHT: synthesis returns row r = (r + 1) (theta + 2 phi)."""

    def __init__(self, lmax, epsilon):
        self.lmax, self.epsilon = lmax, epsilon
        self.calls = []

    def synthesis(self, loc, alm, spin=0, out=None):
        self.calls.append((np.array(loc), np.array(alm), spin))
        return np.outer(np.arange(1, alm.shape[0] + 1), loc[:, 0] + 2 * loc[:, 1])


@pytest.fixture
def plans(monkeypatch):
    made = {}

    def get(lmax, epsilon=1e-12):
        return made.setdefault((lmax, epsilon), _Recorder(lmax, epsilon))

    monkeypatch.setattr(discrete, "get_point_sht", get)
    return made


def _nlm(lmax):
    return (lmax + 1) * (lmax + 2) // 2


def test_degrees_become_colatitude_and_longitude(plans):
    lmax = 5
    lon = np.array([0.0, 90.0, -90.0, 360.0, 725.0, 180.0])
    lat = np.array([90.0, -90.0, 0.0, 45.0, -30.0, 60.0])
    alm = np.ones((2, _nlm(lmax)), dtype=np.complex128)
    got = HipDiscreteMapper(lmax).sample(lon, lat, alm, spin=2)
    (key, rec), = plans.items()
    assert key == (lmax, 1e-12)
    (loc, seen, spin), = rec.calls
    assert spin == 2 and seen.dtype == np.complex128 and seen.shape == alm.shape
    assert loc.shape == (6, 2) and loc.dtype == np.float64
    assert np.array_equal(loc[:, 0], np.radians(90.0 - lat))
    assert np.array_equal(loc[:, 1], np.radians(lon % 360.0))
    assert loc[:, 0].min() == 0.0 and loc[:, 0].max() == np.pi and (loc[:, 1] >= 0).all() and (loc[:, 1] < 2 * np.pi).all()
    assert got.shape == (2, 6)
    assert np.array_equal(got[1], 2 * got[0])


def test_complex64_selects_the_single_precision_object(plans):
    lmax = 4
    mapper = HipDiscreteMapper(lmax, dtype=np.complex64)
    mapper.sample([10.0], [20.0], mapper.create(1))
    mapper.sample([10.0], [20.0], np.zeros((1, _nlm(lmax)), dtype=np.complex128))
    mapper.sample([10.0], [20.0], np.zeros((1, _nlm(lmax))))  # real alms count as double precision
    assert sorted(plans) == [(lmax, 1e-12), (lmax, 1e-5)]
    assert len(plans[lmax, 1e-5].calls) == 1 and len(plans[lmax, 1e-12].calls) == 2


def test_one_dimensional_alm_gives_one_dimensional_values(plans):
    lmax = 3
    lon, lat = np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0, 6.0])
    one = HipDiscreteMapper(lmax).sample(lon, lat, np.zeros(_nlm(lmax), dtype=complex))
    assert one.shape == (3,)
    (loc, seen, spin), = plans[lmax, 1e-12].calls
    assert seen.shape == (1, _nlm(lmax)) and spin == 0
    assert np.array_equal(one, loc[:, 0] + 2 * loc[:, 1])
    assert HipDiscreteMapper(lmax).sample(lon, lat, np.zeros((4, _nlm(lmax)), dtype=complex)).shape == (4, 3)
    assert HipDiscreteMapper(lmax).sample([], [], np.zeros((2, _nlm(lmax)), dtype=complex)).shape == (2, 0)


def test_another_band_limit_is_refused(plans):
    mapper = HipDiscreteMapper(6)
    for bad in (np.zeros(_nlm(5), dtype=complex), np.zeros((2, _nlm(7)), dtype=complex), np.zeros((2, 2, _nlm(6)), dtype=complex)):
        with pytest.raises(ValueError):
            mapper.sample([0.0], [0.0], bad)
    assert not plans


def test_point_field_is_exported():
    import heracles_amd

    assert "PointField" in heracles_amd.__all__ and heracles_amd.PointField is discrete.PointField
