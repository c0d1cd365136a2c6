"""Host logic of HEALPix transforms for fields of any spin weight, with a stub in place of the plan: how ``transform_many`` /
``Plan.map2alm_list`` route the spins, which filter every spin gets, the order of the results and the texts of the errors.  No GPU,
and the library is never loaded."""
import numpy as np
import pytest

from heracles_amd import sht
from heracles_amd.mapper import HipHealpixMapper

NSIDE, LMAX = 4, 6
NPIX, NLM = 12 * NSIDE**2, (LMAX + 1) * (LMAX + 2) // 2


class StubPlan(sht.Plan):
    """The routing of the real ``Plan.map2alm_list`` over recorded calls: a result is filled with 100 i + the spin, where i is the
    number of the call."""

    def __init__(self):
        self.nside, self.lmax, self.npix, self.nlm = NSIDE, LMAX, NPIX, NLM
        self._h = None
        self.calls = []

    def _result(self, shape, spin, out):
        res = np.empty(shape, dtype=complex) if out is None else out
        res[...] = 100 * len(self.calls) + spin
        return res

    def _map2alm_list(self, maps, spins, *, outs=None, fl0=None, fl2=None, niter=0, **kw):
        self.calls.append(("list", list(spins), fl0, fl2, niter))
        return [self._result(((NLM,) if s == 0 else (2, NLM)), s, None if outs is None else outs[i]) for i, s in enumerate(spins)]

    def map2alm(self, maps, spin=0, *, fl=None, niter=0, out=None, **kw):
        self.calls.append(("one", spin, fl, None, niter))
        return self._result(tuple(maps.shape[:-1]) + (NLM,), spin, out)


@pytest.fixture
def stub(monkeypatch):
    plan = StubPlan()
    monkeypatch.setattr(sht, "get_plan", lambda nside, lmax: plan)
    return plan


def _maps(mapper, spins):
    rng = np.random.default_rng(3)
    out = []
    for sp in spins:
        m = mapper.create(*(() if sp == 0 else (2,)), spin=sp)
        m[...] = rng.standard_normal(m.shape)
        out.append(m)
    return out


def test_transform_many_routes_by_spin_and_keeps_the_order(stub):
    w0, w1, w2 = (np.linspace(1.0, 0.5 + 0.1 * k, LMAX + 1) for k in range(3))
    mapper = HipHealpixMapper(NSIDE, LMAX, pixwin={0: w0, 1: w1, 2: w2}, niter=2, ring_weights=np.ones(2 * NSIDE))
    spins = [1, 0, 3, 2, 1]
    maps = _maps(mapper, spins)
    with pytest.raises(ValueError, match="spin-3"):  # no window for spin 3: nothing is transformed
        mapper.transform_many(maps, spins)
    assert stub.calls == []
    spins, maps = spins[:2] + spins[3:], maps[:2] + maps[3:]
    got = mapper.transform_many(maps, spins)
    # one list call for the spin-0 and spin-2 maps, in their order, then one call per field of another weight
    assert [c[:2] for c in stub.calls] == [("list", [0, 2]), ("one", 1), ("one", 1)]
    assert all(c[4] == 2 for c in stub.calls)
    fl0, fl2 = stub.calls[0][2], stub.calls[0][3]
    for fl, w, s in ((fl0, w0, 0), (fl2, w2, 2), (stub.calls[1][2], w1, 1), (stub.calls[2][2], w1, 1)):
        want = np.ones(LMAX + 1)
        want[s:] /= w[s:]
        np.testing.assert_array_equal(fl, want)
    # results in the order of the input, each with its map's metadata
    assert [int(a.flat[0].real) for a in got] == [201, 100, 102, 301]
    assert [a.shape for a in got] == [(2, NLM), (NLM,), (2, NLM), (2, NLM)]
    for a, m, sp in zip(got, maps, spins):
        assert a.dtype.metadata == {**m.dtype.metadata, "deconv": True} and a.dtype.metadata["spin"] == sp


def test_spin0_and_spin2_alone_take_the_list_call_as_before(stub):
    mapper = HipHealpixMapper(NSIDE, LMAX, deconvolve=False, niter=0, ring_weights=np.ones(2 * NSIDE))
    mapper.transform_many(_maps(mapper, [2, 0, 0]), [2, 0, 0])
    assert stub.calls == [("list", [2, 0, 0], None, None, 0)]


def test_transform_passes_any_spin_with_two_components(stub):
    mapper = HipHealpixMapper(NSIDE, LMAX, deconvolve=False, niter=1, ring_weights=np.ones(2 * NSIDE))
    (m,) = _maps(mapper, [3])
    alm = mapper.transform(m, spin=3)
    assert stub.calls == [("one", 3, None, None, 1)]
    assert alm.shape == (2, NLM) and alm.dtype.metadata == {**m.dtype.metadata, "deconv": False}


def test_error_texts(stub):
    plain = HipHealpixMapper(NSIDE, LMAX, deconvolve=False)
    two = np.zeros((2, NPIX))
    with pytest.raises(NotImplementedError, match="spin-1 maps not yet supported"):
        plain.transform(np.zeros(NPIX), spin=1)  # no two-component axis
    with pytest.raises(NotImplementedError, match="spin-3 maps not yet supported"):
        plain.transform(np.zeros((3, NPIX)), spin=3)
    with pytest.raises(NotImplementedError, match="spin--2 maps not yet supported"):
        plain.transform(two, spin=-2)
    with pytest.raises(NotImplementedError, match="spin--1 maps not yet supported"):
        plain.transform_many([two], [-1])
    w = np.ones(LMAX + 1)
    for pixwin in ((w, w), {0: w, 2: w}):  # the spin-2 window is never used for another weight
        with pytest.raises(ValueError, match=r"no pixel window for spin-1 fields.*deconvolve=False.*pixwin=\{1: \.\.\.\}"):
            HipHealpixMapper(NSIDE, LMAX, pixwin=pixwin).transform(two, spin=1)
    with pytest.raises(ValueError, match="shorter than lmax"):
        HipHealpixMapper(NSIDE, LMAX, pixwin={1: w[:-1]}).transform(two, spin=1)
    assert stub.calls == []
    # the list entry point of the library serves 0 and 2 only: the check comes before the library is loaded
    with pytest.raises(NotImplementedError, match="spin-1 maps not yet supported"):
        sht.Plan._map2alm_list(stub, [two], [1])
