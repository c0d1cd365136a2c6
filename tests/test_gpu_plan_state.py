"""What a plan keeps per spin weight -- recursion tables, seed factors and task sets by ring blocks per task, one store per (weight,
kernel family), built on first use (hx_plan::SpinData, spin_data / task_set in hx_plan.hip) -- must not depend on what the plan did
before: a list of calls that between them ask for every family and every block count runs in order on one plan, in reverse order
on a second, and each call alone on a plan of its own; every result must be the same bit for bit.  A collision of keys (two block
counts, spin 2 on its own kernels and through the run-time-spin sweep, tables built for one family and read by another) shows as a
difference between the orderings.  nside 256 / lmax 383: 16 ring blocks, so that tasks of 4, 8 and 16 ring blocks are different lists."""
import contextlib
import os

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu
NSIDE, LMAX = 256, 383
NPIX = 12 * NSIDE * NSIDE


@contextlib.contextmanager
def _generic_spin2():
    """HX_SPIN_GENERIC=1 (read on every call): spin 2 through the run-time-spin sweep."""
    os.environ["HX_SPIN_GENERIC"] = "1"
    try:
        yield
    finally:
        del os.environ["HX_SPIN_GENERIC"]


def _inputs():
    import torch

    rng = np.random.default_rng(256383)
    maps = torch.as_tensor(rng.standard_normal((10, NPIX))).cuda()
    alm0 = torch.as_tensor(helpers.random_alm(rng, LMAX, 0, (5,))).cuda()
    alm2 = torch.as_tensor(helpers.random_alm(rng, LMAX, 2, (3, 2))).cuda()
    alm3 = torch.as_tensor(helpers.random_alm(rng, LMAX, 3, (2,))).cuda()
    return maps, alm0, alm2, alm3


def _calls(maps, alm0, alm2, alm3):
    def generic(plan):
        with _generic_spin2():
            return plan.map2alm(maps[:2], 2)

    return [
        ("spin-0 one map", lambda p: p.map2alm(maps[:1], 0)),
        ("spin-0 ten maps", lambda p: p.map2alm(maps, 0)),
        ("spin-2 one field", lambda p: p.map2alm(maps[:2], 2)),
        ("spin-2 five fields", lambda p: p.map2alm(maps.reshape(5, 2, NPIX), 2)),
        ("spin-2 via HX_SPIN_GENERIC=1", generic),
        ("spin 1", lambda p: p.map2alm(maps[:2], 1)),
        ("alm2map five maps", lambda p: p.alm2map(alm0, 0)),
        ("alm2map three fields", lambda p: p.alm2map(alm2, 2)),
        ("alm2map spin 3", lambda p: p.alm2map(alm3, 3)),
    ]


@pytest.fixture(scope="module")
def results():
    """{ordering: {call: result}} for the orderings "forward", "reverse" and "alone"; computed once, never written."""
    import heracles_amd as hx

    calls = _calls(*_inputs())
    out = {"forward": {}, "reverse": {}, "alone": {}}
    for ordering, seq in (("forward", calls), ("reverse", calls[::-1])):
        plan = hx.Plan(NSIDE, LMAX)
        for name, fn in seq:
            out[ordering][name] = fn(plan).cpu().numpy()
        plan.close()
    for name, fn in calls:
        plan = hx.Plan(NSIDE, LMAX)
        out["alone"][name] = fn(plan).cpu().numpy()
        plan.close()
    for d in out.values():
        for a in d.values():
            a.setflags(write=False)
    return out


def test_every_call_ran_and_gave_something(results):
    assert len(results["forward"]) == len(results["reverse"]) == len(results["alone"]) == 9
    for name, a in results["alone"].items():
        assert np.isfinite(a.view(np.float64)).all() and np.abs(a).max() > 0, name


def test_order_of_first_use_does_not_change_a_bit(results):
    for name, a in results["forward"].items():
        assert np.array_equal(a, results["reverse"][name]), name


def test_a_used_plan_gives_what_a_fresh_one_gives(results):
    for name, a in results["alone"].items():
        assert np.array_equal(a, results["forward"][name]), name
        assert np.array_equal(a, results["reverse"][name]), name


def test_generic_spin2_agrees_with_its_own_kernels(results):
    """Seeds and tables of the two families round differently (tests/test_gpu_healpix_spin.py: 1e-12 of the largest alm); they need
    not differ."""
    for ordering, d in results.items():
        a, g = d["spin-2 one field"], d["spin-2 via HX_SPIN_GENERIC=1"]
        err = np.abs(g - a).max() / np.abs(a).max()
        print(f"{ordering}: generic against specialised spin 2: {err:.3e}")
        assert err < 1e-12, ordering
