"""A plain ``bench.py`` run measures the headline figure only, and ``--dump-outputs`` writes what its timed path returned in the last
step: the Cl rows and (at N = 1) a seeded sample of the alms -- at these sizes all of them, so the rows can be re-derived from them."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSIDE, LMAX, NBINS = 64, 96, 2


def _bench(args, env=None, timeout=600):
    env = dict(os.environ if env is None else env)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=timeout)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _small(steps=2, warmup=1):
    return ["--steps", str(steps), "--warmup", str(warmup), "--nside", str(NSIDE), "--lmax", str(LMAX), "--nbins", str(NBINS)]


def test_plain_run_is_the_headline_and_dumps_what_it_computed(tmp_path):
    from heracles_amd.distributed import ShardedTwoPoint

    nlm = (LMAX + 1) * (LMAX + 2) // 2
    spins = [0] * NBINS + [2] * NBINS
    work = ShardedTwoPoint(spins, 1, 0, nlm, LMAX, kernel=lambda *a: None)
    outs = []
    for run in ("a", "b"):
        out = _bench(["--gpus", "1", *_small(), "--dump-outputs", str(tmp_path / run)])
        assert out["metric"].startswith("map->Cl pairs/sec") and out["unit"] == "map->Cl pairs/s" and out["higher_is_better"] is True
        assert out["dtype"] == "f64" and out["value"] > 0 and out["steps"] == 2 and out["warmup"] == 1
        assert out["ms_per_step"] == pytest.approx(len(work.pairs) * 1e3 / out["value"], rel=1e-9)
        # every leg beyond the headline is --full only
        for k in ("verify", "cpu_baseline", "host_to_host", "niter3", "single_map_transforms", "mixmat", "mixmat_list", "roofline",
                  "measured_peaks", "verified"):
            assert out[k] is None, k
        files = {f: np.load(tmp_path / run / f"{f}.npy") for f in ("cl", "alm_spin0_sample", "alm_spin2_sample")}
        assert sum(os.path.getsize(tmp_path / run / f"{f}.npy") for f in files) <= 64 << 20
        assert all(a.dtype == np.float64 for a in files.values())
        assert files["cl"].shape == (work.nrows, LMAX + 1)
        assert files["alm_spin0_sample"].shape == (NBINS * nlm, 2) and files["alm_spin2_sample"].shape == (2 * NBINS * nlm, 2)
        outs.append(files)
    # the same arguments give the same inputs, hence the same outputs
    for f in outs[0]:
        np.testing.assert_allclose(outs[1][f], outs[0][f], rtol=1e-12, atol=1e-14 * np.abs(outs[0][f]).max())
    # the dumped rows are the spectra of the dumped alms: auto spectrum of the first spin-0 map by a direct sum
    cl, a = outs[0]["cl"], outs[0]["alm_spin0_sample"].reshape(NBINS, nlm, 2)[0]
    ell = np.concatenate([np.arange(m, LMAX + 1) for m in range(LMAX + 1)])
    w = np.where(np.arange(nlm) <= LMAX, 1.0, 2.0)
    ref = np.bincount(ell, weights=w * (a[:, 0] ** 2 + a[:, 1] ** 2), minlength=LMAX + 1) / (2.0 * np.arange(LMAX + 1) + 1.0)
    np.testing.assert_allclose(cl[work.row0[0, 0]], ref, rtol=1e-11, atol=1e-14 * np.abs(ref).max())


def test_plain_two_rank_rehearsal_times_the_fixed_job_only(tmp_path):
    """At N > 1 a plain run times the fixed job through both routes (`value` = the better one) and nothing else; the rows of that
    route are what --dump-outputs writes."""
    env = dict(os.environ, HX_BENCH_SHARE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    out = _bench(["--gpus", "2", *_small(steps=1, warmup=0), "--dump-outputs", str(tmp_path)], env=env)
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["config"]["pairs"] == 10
    assert out["value"] == max(out["routes"]["m_sharded"]["value"], out["routes"]["all_gather"]["value"]) > 0
    assert out["weak_scaling"] is None and out["value_weak"] is None and out["verify_multi"] is None and out["verified"] is None
    cl = np.load(tmp_path / "cl.npy")
    assert cl.dtype == np.float64 and cl.shape[1] == LMAX + 1 and np.isfinite(cl).all() and np.abs(cl).max() > 0
