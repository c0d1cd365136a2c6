"""Lead-in table of the batched Legendre analysis (k_legendre_duo, hx_analysis.hip): a ring group resumes its recursion chains at the
first pair of 32-l blocks in which one of its waves issues matrix instructions, from states that a scout instantiation of the same
kernel stored in HBM, instead of running seeds and lead-in again in every sweep.  Nothing but the vector work may change: the alms
are the same BITS with the table and without, on every route of the analysis, the matrix instructions issued are the same number and
the vector flops fall.  By default (hx_plan_set_leadin_resume 1) only the spin-2 sweeps keep a table; the spin-0 sweeps, which it does
not make faster, read one only when the plan asks for it (2), and that is what these tests switch on.

Group-level lead-ins need more than one ring group per order.  nside 256 / lmax 767 has four groups of four ring blocks (spin 2) per
order; its polar groups wake blocks late and never wake near the pruning limit (first groups that write zeros only, later groups
that do nothing).  Its two spin-0 groups of eight ring blocks have NO lead-in: the polar one ends at ring pair 255 (sin theta = 0.745),
which is pruned above m = 671, where its seed 0.745^671 ~ 1e-86 is still above the 2^-300 of the spin-0 chains -- both groups issue
matrix instructions in block 0, the table holds b_res = 0 throughout and the vector flops are EQUAL (measured: 6.229524e+08 both ways).
The spin-0 path is therefore held at nside 512 / lmax 1535 as well: four groups, the polar one ends at sin theta = 0.40 and wakes
eight or more blocks late.  nside 256 / lmax 383 and nside 128 / lmax 383 are the shapes of the other plan tests.
Sweep shapes <SPIN, NG, NBX, NSUB>: 8 / 10 / 16 spin-0 maps = <0,1,0,2>, <0,1,1,2>, <0,2,0,1>; 3 / 5 / 10 spin-2 fields = <2,1,0,2>,
<2,1,1,2>, <2,2,2,1>."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANS = [(256, 767), (256, 383), (128, 383), (512, 1535)]
LEADIN_PLAN = {2: (256, 767), 0: (512, 1535)}  # the smallest plan whose ring groups of that spin have lead-ins (see above)
SHAPES = [(0, 8), (0, 10), (0, 16), (2, 3), (2, 5), (2, 10)]  # (spin, maps or fields)

_cache = {}


def _maps(nside):
    """Twenty maps of a resolution on the device, made once and never written."""
    import torch

    if ("maps", nside) not in _cache:
        rng = np.random.default_rng(4096 + nside)
        _cache["maps", nside] = torch.as_tensor(rng.standard_normal((20, 12 * nside * nside))).cuda()
    return _cache["maps", nside]


def _weights(nside, lmax):
    import torch

    if ("w", nside, lmax) not in _cache:
        rng = np.random.default_rng(17 + nside + lmax)
        pw = torch.as_tensor(1.0 + 1e-2 * rng.standard_normal(12 * nside * nside)).cuda()
        fl = torch.as_tensor(1.0 + 1e-2 * rng.standard_normal(lmax + 1)).cuda()
        _cache["w", nside, lmax] = (pw, fl)
    return _cache["w", nside, lmax]


def _plan(nside, lmax):
    import heracles_amd as hx

    if ("plan", nside, lmax) not in _cache:
        _cache["plan", nside, lmax] = hx.Plan(nside, lmax)
    return _cache["plan", nside, lmax]


def _input(nside, spin, n):
    maps = _maps(nside)
    return maps[:n] if spin == 0 else maps[: 2 * n].reshape(n, 2, -1)


def _on_off(plan, fn):
    """fn() with the tables of both spins and without, as host arrays, with the (matrix, vector) flops each call executed."""
    import heracles_amd as hx

    out = {}
    for on in (True, False):
        plan.set_leadin_resume(on, spin0=True)
        hx._lib.executed_flops(reset=True)
        a = fn()
        a = [x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in (a if isinstance(a, (list, tuple)) else [a])]
        out[on] = (a, hx._lib.executed_flops(reset=True))
    plan.set_leadin_resume(True)
    return out


def _assert_same_bits(out, what):
    (a_on, _), (a_off, _) = out[True], out[False]
    assert len(a_on) == len(a_off)
    for x, y in zip(a_on, a_off):
        assert np.isfinite(x.view(np.float64)).all() and np.abs(x).max() > 0, what
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("spin,n", SHAPES)
@pytest.mark.parametrize("nside,lmax", PLANS)
def test_alms_are_the_same_bits_with_and_without_the_table(nside, lmax, spin, n):
    """Plain sweeps, sweeps with pixel weights and a filter, and the Jacobi iteration (niter = 1: the second analysis ADDS to the alms)."""
    plan = _plan(nside, lmax)
    maps = _input(nside, spin, n)
    pw, fl = _weights(nside, lmax)
    _assert_same_bits(_on_off(plan, lambda: plan.map2alm(maps, spin)), "plain")
    _assert_same_bits(_on_off(plan, lambda: plan.map2alm(maps, spin, pix_weights=pw, fl=fl)), "pixel weights and fl")
    _assert_same_bits(_on_off(plan, lambda: plan.map2alm(maps, spin, niter=1)), "niter = 1")


@pytest.mark.parametrize("spin,n", SHAPES)
@pytest.mark.parametrize("nside,lmax", [(256, 767), (512, 1535)])
def test_same_matrix_work_less_vector_work(nside, lmax, spin, n):
    """hx_executed_flops of one call: the matrix instructions issued are the same number, the recursion blocks run are fewer --
    strictly, wherever the plan has lead-ins to skip (all but spin 0 at nside 256 / lmax 767: see above)."""
    plan = _plan(nside, lmax)
    maps = _input(nside, spin, n)
    out = _on_off(plan, lambda: plan.map2alm(maps, spin))
    (mf_on, v_on), (mf_off, v_off) = out[True][1], out[False][1]
    print(f"spin {spin}, {n} units: matrix flops {mf_on:.6e} / {mf_off:.6e}, vector flops {v_on:.6e} / {v_off:.6e}, ratio {v_on / v_off:.4f}")
    assert mf_on == mf_off and mf_on > 0
    if spin == 0 and (nside, lmax) == (256, 767):
        assert v_on == v_off
    else:
        assert v_on < v_off
    _assert_same_bits(out, "counted call")


@pytest.mark.parametrize("spin,n", [(0, 10), (2, 10)])
def test_m_chunks(spin, n):
    """A scratch budget that cuts the sweep into three or more m-chunks: every chunk indexes the one table of the task set."""
    import heracles_amd as hx

    nside, lmax = LEADIN_PLAN[spin]
    plan = _plan(nside, lmax)
    maps = _input(nside, spin, n)
    whole = plan.map2alm(maps, spin).cpu().numpy()
    hx._lib.set_scratch_budget(40e6 if nside == 256 else 120e6)  # (the operands of all orders: 250 / 500 MB)
    try:
        out = _on_off(plan, lambda: plan.map2alm(maps, spin))
        assert plan.last_chunks >= 3, plan.last_chunks
    finally:
        hx._lib.set_scratch_budget(0)
    _assert_same_bits(out, "chunked")
    assert np.array_equal(out[True][0][0], whole)
    assert out[True][1][1] < out[False][1][1]


def test_streamed_sweeps_of_host_maps():
    """hx_map2alm_multi on host maps: the rings arrive in slabs and every ring group ADDS to rows that were cleared (no first group that
    stores); the per-slab task tables index the same task list and table.  That the call streamed shows in the Legendre launches: one
    per slab of rings (twelve slabs by default) where the fallback, whole maps in sweeps of five fields / eight maps, has two per spin
    and only one batched sweep of spin 0."""
    import heracles_amd as hx

    nside, lmax = LEADIN_PLAN[0]
    plan = _plan(nside, lmax)
    m2 = _input(nside, 2, 10).cpu().numpy()
    m0 = _input(nside, 0, 10).cpu().numpy()
    hx._lib.profile_enable(True)
    try:
        hx._lib.profile_reset()
        out = _on_off(plan, lambda: plan.map2alm_multi([(m2, 2, None), (m0, 0, None)]))
        launches = [hx._lib.profile_get(f"legendre_analysis_s{s}")[0] for s in (2, 0)]
    finally:
        hx._lib.profile_enable(False)
    print("Legendre launches of the two calls, spin 2 / spin 0:", launches)
    assert min(launches) >= 2 * 3, launches
    _assert_same_bits(out, "streamed")
    assert out[True][1][0] == out[False][1][0] and out[True][1][1] < out[False][1][1]


@pytest.mark.parametrize("spin,n", [(0, 10), (2, 10)])
def test_m_sharded_route(spin, n):
    """hx_legendre_from_modes on the orders q, q + 3, q + 6, ... (m_step 3): sweeps over a subset of the orders, same table."""
    from heracles_amd.distributed import HipStages, order_sets

    nside, lmax = LEADIN_PLAN[spin]
    plan = _plan(nside, lmax)
    st = HipStages(plan)
    maps = _input(nside, spin, n).reshape(-1, 12 * nside * nside)
    ncomp = maps.shape[0]
    sets = order_sets(lmax, 3)
    assert all(s[2] == 3 for s in sets)
    blocks = st.ring_modes(maps, sets)

    def run():
        alm = st.zeros_alm(ncomp, plan.nlm)
        for q, orders in enumerate(sets):
            size = st.modes_size(orders[1])
            st.legendre(spin, [blocks[q][c * size : (c + 1) * size] for c in range(ncomp)], orders, alm)
        return alm

    out = _on_off(plan, run)
    _assert_same_bits(out, "m-sharded")
    assert out[True][1][0] == out[False][1][0] and out[True][1][1] < out[False][1][1]


@pytest.mark.parametrize("spin,n", [(0, 10), (2, 10)])
def test_the_table_is_scratch_and_capped(spin, n):
    """hx_plan_scratch_bytes counts the table, hx_plan_release_scratch drops it and the next call builds it again; with the cap forced
    below its size the call runs from the seeds, as with the switch off."""
    import heracles_amd as hx

    nside, lmax = LEADIN_PLAN[spin]
    plan = hx.Plan(nside, lmax)
    maps = _input(nside, spin, n)

    def call():
        hx._lib.executed_flops(reset=True)
        a = plan.map2alm(maps, spin).cpu().numpy()
        return a, hx._lib.executed_flops(reset=True)

    plan.set_leadin_resume(False)
    ref, (mf_off, v_off) = call()
    bytes_off = plan.scratch_bytes
    plan.set_leadin_resume(True, cap_bytes=1024, spin0=True)  # no table fits
    a, (mf, v) = call()
    assert np.array_equal(a, ref) and (mf, v) == (mf_off, v_off)
    assert plan.scratch_bytes == bytes_off
    plan.set_leadin_resume(True, cap_bytes=0, spin0=True)  # the default cap
    a, (mf, v_on) = call()
    assert np.array_equal(a, ref) and mf == mf_off and v_on < v_off
    bytes_on = plan.scratch_bytes
    per_group = 10240 if spin == 0 else 5120
    assert bytes_on > bytes_off and (bytes_on - bytes_off) % per_group == 0
    plan.release_scratch()
    assert plan.scratch_bytes < bytes_off
    a, (mf, v) = call()
    assert np.array_equal(a, ref) and (mf, v) == (mf_off, v_on)
    assert plan.scratch_bytes == bytes_on
    plan.close()


def test_spin0_table_only_on_request():
    """The default switch builds the spin-2 table and no spin-0 table: a spin-0 sweep then runs the vector work of the switch off
    and adds nothing to the plan's scratch."""
    import heracles_amd as hx

    nside, lmax = LEADIN_PLAN[0]
    plan = hx.Plan(nside, lmax)

    def call(spin):
        hx._lib.executed_flops(reset=True)
        a = plan.map2alm(_input(nside, spin, 10), spin).cpu().numpy()
        return a, hx._lib.executed_flops(reset=True)

    plan.set_leadin_resume(False)
    ref0, flops0 = call(0)
    ref2, flops2 = call(2)
    bytes_off = plan.scratch_bytes
    plan.set_leadin_resume(True)  # the default
    a0, f0 = call(0)
    assert np.array_equal(a0, ref0) and f0 == flops0 and plan.scratch_bytes == bytes_off
    a2, f2 = call(2)
    assert np.array_equal(a2, ref2) and f2[0] == flops2[0] and f2[1] < flops2[1] and plan.scratch_bytes > bytes_off
    plan.close()
