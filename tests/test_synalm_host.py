"""Host side of the Gaussian mocks (no GPU): the shared Philox header compiled for the host, the numpy reference of the definition
(tests/synalm_reference.py) pinned on its own, and the key / shape logic of ``hx.synalm`` with the library call stubbed out."""

import os
import re
import subprocess

import numpy as np
import pytest

import synalm_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_header_on_the_host(tmp_path):
    exe = tmp_path / "t_philox"
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "csrc", "test_philox.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout


# ---- the reference, pinned on its own -------------------------------------------------------------------------------------------------

def test_reference_philox_known_answers():
    for counter, key, want in sr.KNOWN_ANSWERS:
        got = tuple(int(x) for x in sr.philox4x32_10(*counter, *key))
        assert got == want


def test_reference_uniform_edges():
    z, o = np.uint64(0), np.uint64(0xFFFFFFFF)
    assert sr.uniforms(z, z, z, z) == (2.0**-53, 0.0)
    assert sr.uniforms(o, o, o, o) == (1.0, 1.0 - 2.0**-53)


@pytest.mark.parametrize("ncomp,lmax", [(1, 4), (3, 33), (9, 70)])
def test_reference_factor(ncomp, lmax):
    C = sr.conditioned_spectra(ncomp, lmax, 3)
    L = sr.unpack(sr.cholesky(sr.pack(C), ncomp), ncomp, lower=True)
    assert (L[np.triu_indices(ncomp, 1)] == 0).all()
    np.testing.assert_allclose(np.einsum("ikl,jkl->ijl", L, L), C, rtol=1e-12, atol=0)


def test_reference_factor_tau_rule():
    nl = 12
    c = 4.0 ** -(np.arange(nl) % 6)
    C = np.broadcast_to(c, (2, 2, nl)).copy()  # two identical components: the second pivot is exactly 0
    L = sr.unpack(sr.cholesky(sr.pack(C), 2), 2, lower=True)
    assert (L[1, 1] == 0).all() and (L[1, 0] == L[0, 0]).all() and (L[0, 0] == 2.0 ** -(np.arange(nl) % 6)).all()
    bad = np.zeros((2, 2, 6))
    bad[:, :, 3] = [[1, 2], [2, 1]]
    with pytest.raises(ValueError, match="l = 3"):
        sr.cholesky(sr.pack(bad), 2)
    with pytest.raises(ValueError, match="NaN"):
        sr.cholesky(np.array([[1.0, np.nan]]), 1)


def test_reference_alms_are_prefix_consistent_and_real_at_m0():
    C5 = np.broadcast_to(np.eye(2)[:, :, None], (2, 2, 6)).copy()
    a5, a1 = sr.synalm(sr.pack(C5), 2, 1 << 33), sr.synalm(sr.pack(C5[..., :2]), 2, 1 << 33)
    l5, m5 = sr.lm_index(5)
    assert (a5[:, m5 == 0].imag == 0).all()
    assert (a5[:, l5 <= 1] == a1).all()


def test_reference_spectra_statistics():
    C = sr.roundtrip_matrix()
    alms = sr.synalm(sr.pack(C), C.shape[0], sr.ROUNDTRIP_SEED)
    sr.assert_spectra_statistics(C, sr.alm2cl_matrix(alms))


def test_round_trip_helpers_invert_each_other():
    C = sr.roundtrip_matrix()
    cls = sr.matrix_to_cls(C, sr.ROUNDTRIP_FIELDS)
    assert cls["POS", "POS", 1, 2].shape == (131,) and cls["POS", "SHE", 2, 1].shape == (2, 131) and cls["SHE", "SHE", 1, 2].shape == (2, 2, 131)
    assert (sr.cls_to_matrix(cls, sr.ROUNDTRIP_FIELDS) == C).all()


# ---- hx.synalm: host logic with the launch stubbed out ----------------------------------------------------------------------------------

@pytest.fixture
def stub(monkeypatch):
    """Replace the library call: records the packed spectra, returns alms whose row r is filled with r."""
    from heracles_amd import mocks

    calls = []

    def fake(cl, ncomp, *, seed, realisation=0, out=None):
        calls.append({"cl": np.array(cl), "ncomp": ncomp, "seed": seed, "realisation": realisation})
        lmax = cl.shape[1] - 1
        return np.arange(ncomp)[:, None] * np.ones((lmax + 1) * (lmax + 2) // 2, dtype=np.complex128)

    monkeypatch.setattr(mocks, "synalm_components", fake)
    return calls


def _spin(block, s1, s2):
    block = np.array(block, dtype=float)
    block.dtype = np.dtype(block.dtype.str, metadata={"spin_1": s1, "spin_2": s2})
    return block


def test_synalm_key_order_shapes_and_spins(stub):
    import heracles_amd as hx

    C = sr.roundtrip_matrix()
    cls = sr.matrix_to_cls(C, sr.ROUNDTRIP_FIELDS)
    alms = hx.synalm(cls, seed=11, realisation=3)
    assert list(alms) == [("POS", 1), ("POS", 2), ("SHE", 1), ("SHE", 2)]
    nlm = 131 * 132 // 2
    assert [a.shape for a in alms.values()] == [(nlm,), (nlm,), (2, nlm), (2, nlm)]
    assert [a.dtype.metadata["spin"] for a in alms.values()] == [0, 0, 2, 2]
    # component numbering follows the order of the auto-spectra in the dict: rows 0, 1, (2, 3), (4, 5)
    assert alms["POS", 2][0] == 1 and (alms["SHE", 2][:, 0] == [4, 5]).all()
    (call,) = stub
    assert call["ncomp"] == 6 and call["seed"] == 11 and call["realisation"] == 3
    assert (call["cl"] == sr.pack(C)).all()
    # the order of the dict is part of the definition: SHE first renumbers the components
    rev = {k: cls[k] for k in reversed(list(cls))}
    alms = hx.synalm(rev, seed=11)
    assert list(alms) == [("SHE", 2), ("SHE", 1), ("POS", 2), ("POS", 1)]
    order = [4, 5, 2, 3, 1, 0]
    assert (stub[-1]["cl"] == sr.pack(C[np.ix_(order, order)])).all()


def test_synalm_result_spin_and_plain_arrays(stub):
    import heracles_amd as hx

    nl = 5
    ee = np.zeros((2, 2, nl))
    ee[0, 0], ee[1, 1], ee[0, 1], ee[1, 0] = 3.0, 2.0, 0.5, 0.5
    cls = {("T", "T", 0, 0): np.full(nl, 7.0), ("G", "G", 0, 0): hx.Result(ee, spin=(1, 1), axis=-1)}
    alms = hx.synalm(cls, seed=1)
    assert alms["T", 0].dtype.metadata["spin"] == 0 and alms["G", 0].dtype.metadata["spin"] == 1
    full = sr.unpack(stub[-1]["cl"], 3)
    assert (full[0, 0] == 7).all() and (full[1, 1] == 3).all() and (full[2, 2] == 2).all() and (full[1, 2] == 0.5).all()
    assert (full[0, 1] == 0).all() and (full[0, 2] == 0).all()  # a missing cross-spectrum is zero
    with pytest.raises(ValueError, match="no spin"):
        hx.synalm({("G", "G", 0, 0): ee}, seed=1)


def test_synalm_swapped_cross_key_is_transposed(stub):
    import heracles_amd as hx

    nl = 4
    tt, ee = np.full(nl, 4.0), _spin(np.zeros((2, 2, nl)), 2, 2)
    ee[0, 0] = ee[1, 1] = 5.0
    te = _spin(np.stack([np.full(nl, 1.0), np.full(nl, -2.0)]), 0, 2)  # (T x E, T x B)
    straight = {("T", "T", 0, 0): tt, ("G", "G", 0, 0): ee, ("T", "G", 0, 0): te}
    swapped = {("T", "T", 0, 0): tt, ("G", "G", 0, 0): ee, ("G", "T", 0, 0): _spin(te, 2, 0)}
    hx.synalm(straight, seed=1)
    hx.synalm(swapped, seed=1)
    assert (stub[0]["cl"] == stub[1]["cl"]).all()
    full = sr.unpack(stub[0]["cl"], 3)
    assert (full[0, 1] == 1).all() and (full[0, 2] == -2).all() and (full[1, 2] == 0).all()
    # two spin-2 fields: the swapped block is the transpose over the component axes
    gg = _spin(np.arange(4.0).reshape(2, 2, 1) * np.ones(nl), 2, 2)
    hx.synalm({("G", "G", 0, 0): ee, ("G", "G", 1, 1): ee, ("G", "G", 0, 1): gg}, seed=1)
    hx.synalm({("G", "G", 0, 0): ee, ("G", "G", 1, 1): ee, ("G", "G", 1, 0): _spin(gg.transpose(1, 0, 2), 2, 2)}, seed=1)
    assert (stub[2]["cl"] == stub[3]["cl"]).all()
    assert (sr.unpack(stub[2]["cl"], 4)[1, 2] == 2).all()  # B of bin 0 x E of bin 1 = gg[1, 0]


def test_synalm_missing_auto_and_short_spectra_raise(stub):
    import heracles_amd as hx

    nl = 6
    with pytest.raises(ValueError, match="auto-spectrum"):
        hx.synalm({("T", "T", 0, 0): np.ones(nl), ("T", "K", 0, 0): np.ones(nl)}, seed=1)
    with pytest.raises(ValueError, match="auto-spectrum"):
        hx.synalm({("T", "K", 0, 0): np.ones(nl)}, seed=1)
    cls = {("T", "T", 0, 0): np.ones(nl), ("K", "K", 0, 0): np.ones(nl + 3), ("T", "K", 0, 0): np.ones(nl + 1)}
    with pytest.raises(ValueError, match="multipoles"):
        hx.synalm(cls, seed=1, lmax=nl)
    hx.synalm(cls, seed=1, lmax=3)  # longer ones are cut
    assert stub[-1]["cl"].shape == (3, 4)
    hx.synalm(cls, seed=1)  # default: the shortest
    assert stub[-1]["cl"].shape == (3, nl)


def test_synalm_components_checks_its_arguments():
    import heracles_amd as hx

    with pytest.raises(ValueError, match="expected"):
        hx.synalm_components(np.ones((2, 4)), 2, seed=1)
    with pytest.raises(ValueError, match="seed"):
        hx.synalm_components(np.ones((1, 4)), 1, seed=2**64)
    with pytest.raises(ValueError, match="realisation"):
        hx.synalm_components(np.ones((1, 4)), 1, seed=1, realisation=-1)
    with pytest.raises(ValueError, match="out has shape"):
        hx.synalm_components(np.ones((1, 4)), 1, seed=1, out=np.empty((1, 9), dtype=complex))


def test_tile_constants_restated_in_python_match_the_kernel():
    from heracles_amd import mocks

    text = open(os.path.join(ROOT, "heracles_amd", "csrc", "hx_synalm.hip")).read()
    for name, value in (("SYN_LT", mocks.TILE_L), ("SYN_MC", mocks.TILE_M), ("SYN_RB", mocks.TILE_COMP), ("SYN_RB_SMALL", mocks.TILE_COMP_SMALL), ("SYN_MAXN", mocks.MAX_COMPONENTS)):
        assert re.search(rf"constexpr int {name} = (\d+);", text).group(1) == str(value)
