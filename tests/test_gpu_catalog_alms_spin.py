"""catalog_alms for complex fields of spin weight 1 and 3 on a HipDiscreteMapper (hx_catalm_finish in front of the run-time-spin
sweep of the point transform), against the long-double direct sum of tests/spin_reference.py: the spin-2 case of
tests/test_gpu_catalog_alms.py with another weight, the same bound (1e-11 of the largest |alm|).  Then the alms go through
transform and angular_power_spectra, which must carry the weights into the Result."""
import numpy as np
import pytest

from discrete_cases import to_point
from spin_reference import points2alm_spin

pytestmark = pytest.mark.gpu

FOUR_PI = 4 * np.pi


def test_spin1_and_spin3_fields_through_catalog_alms():
    import heracles_amd as hx

    class F1(hx.ComplexField, spin=1):
        pass

    class F3(hx.ComplexField, spin=3):
        pass

    lmax, n = 32, 2000
    rng = np.random.default_rng(13)
    c = {"lon": rng.uniform(-180, 540, n), "lat": np.degrees(np.arcsin(rng.uniform(-1, 1, n))),
         "w": rng.uniform(0.5, 1.5, n), "g1": rng.normal(0, 0.3, n), "g2": rng.normal(0, 0.3, n)}
    cat = hx.ArrayCatalog(c, page_size=1000)  # two pages
    m = hx.HipDiscreteMapper(lmax)
    fields = {"D": F1(m, "lon", "lat", "g1", "g2", "w"), "F": F3(m, "lon", "lat", "g1", "g2", "w")}
    alms = hx.catalog_alms(fields, {0: cat})
    theta, phi = to_point(c["lon"], c["lat"])
    wbar = n / FOUR_PI * c["w"].mean()
    rows = np.stack([c["g1"] * c["w"], c["g2"] * c["w"]])
    for name, s in (("D", 1), ("F", 3)):
        got = alms[name, 0]
        want = points2alm_spin(theta, phi, rows, lmax, s) / wbar
        assert got.shape == want.shape == (2, (lmax + 1) * (lmax + 2) // 2)
        err = np.abs(np.asarray(got) - want).max() / np.abs(want).max()
        print(f"{name} (spin {s}): max error {err:.3e} of the largest |alm|")
        assert err < 1e-11
        md = dict(got.dtype.metadata)
        assert (md["geometry"], md["kernel"], md["lmax"], md["spin"]) == ("discrete", "none", lmax, s)
        assert md["wbar"] == pytest.approx(wbar, rel=1e-12)
    cls = hx.angular_power_spectra(hx.transform(fields, alms))
    for name, s in (("D", 1), ("F", 3)):
        res = cls[name, name, 0, 0]
        assert res.spin == (s, s)
        assert np.asarray(res).shape == (2, 2, lmax + 1)
    assert cls["D", "F", 0, 0].spin == (1, 3)


def test_one_component_field_with_a_spin_weight_raises():
    import heracles_amd as hx

    class S1(hx.ScalarField, spin=1):
        pass

    class Fm(hx.ComplexField, spin=-1):
        pass

    m = hx.HipDiscreteMapper(8)
    c = {"lon": np.array([10.0, 20.0]), "lat": np.array([0.0, 5.0]), "v": np.ones(2), "u": np.ones(2)}
    with pytest.raises(ValueError):
        hx.catalog_alms({"S": S1(m, "lon", "lat", "v")}, {0: hx.ArrayCatalog(c, page_size=2)})
    with pytest.raises(ValueError):
        hx.catalog_alms({"F": Fm(m, "lon", "lat", "v", "u")}, {0: hx.ArrayCatalog(c, page_size=2)})
