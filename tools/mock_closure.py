"""Closed loop of the catalogue half of the pipeline on mocks with a known answer: spectra -> gaussian_maps -> mock_catalogs ->
map_catalogs -> transform -> angular_power_spectra(debias=True), at nside 64 (env NSIDE) over 32 realisations (env NREAL), one
Positions bin and one Shears bin with a cross-correlation.

The mock points carry the values of the band-limited maps at their pixels' centres and are mapped back at the same nside, so the
mapped fields are those maps, Poisson-sampled: the expectation of the debiased spectra is the input (the pixel window, which would
enter squared for a field that varies inside a pixel, is 1 here) -- up to the quadrature error of unit pixel weights and, for the
shears, the source-density weighting (1 + delta) gamma of a catalogue whose points follow the density.  Writes the mean spectra, the
standard error of the mean and the input to OUT (default profiles/mock_closure.json), with the largest and rms deviation in units
of the standard error per block.  DESIGN.md 4.16."""

import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import heracles_amd as hx

NSIDE = int(os.environ.get("NSIDE", "64"))
NREAL = int(os.environ.get("NREAL", "32"))
NBAR = float(os.environ.get("NBAR", "4"))
SIGMA = float(os.environ.get("SIGMA", "0.05"))
SEED = int(os.environ.get("SEED", "20241020"))
OUT = os.environ.get("OUT", "profiles/mock_closure.json")


def with_spins(block, s1, s2):
    block = np.array(block, dtype=float)
    block.dtype = np.dtype(block.dtype.str, metadata={"spin_1": s1, "spin_2": s2})
    return block


def input_spectra(lmax):
    l = np.arange(lmax + 1.0)
    pp = 1e-3 / (l + 10.0)
    ee = 2e-5 / (l + 10.0)
    pp[0] = 0.0
    ee[:2] = 0.0
    pe = 0.5 * np.sqrt(pp * ee)
    zero = np.zeros(lmax + 1)
    return {("POS", "POS", 1, 1): with_spins(pp, 0, 0), ("POS", "SHE", 1, 1): with_spins([pe, zero], 0, 2),
            ("SHE", "SHE", 1, 1): with_spins([[ee, zero], [zero, zero]], 2, 2)}


def main():
    warnings.filterwarnings("ignore", message="HipHealpixMapper")
    hx.init(0)
    lmax = 3 * NSIDE // 2
    npix = 12 * NSIDE * NSIDE
    mapper = hx.HipHealpixMapper(NSIDE, lmax, deconvolve=False)
    fields = {"POS": hx.Positions(mapper, "ra", "dec"), "SHE": hx.Shears(mapper, "ra", "dec", "g1", "g2", "w")}
    cls = input_spectra(lmax)
    vis = np.ones(npix)
    runs = {key: [] for key in cls}
    sizes = []
    for r in range(NREAL):
        maps = hx.gaussian_maps(fields, cls, seed=SEED, realisation=r, device="cuda")
        cats = hx.mock_catalogs(fields, maps, NBAR, visibility=vis, noise={"SHE": SIGMA}, seed=SEED, realisation=r)
        sizes.append(cats[1].size)
        data = hx.map_catalogs(fields, cats, device="cuda")
        data = {key: data[key] for key in (("POS", 1), ("SHE", 1))}
        est = hx.angular_power_spectra(hx.transform(fields, data, device="cuda"), debias=True)
        for key in cls:
            runs[key].append(np.asarray(getattr(est[key], "array", est[key]), dtype=float))
    out = {"nside": NSIDE, "lmax": lmax, "realisations": NREAL, "nbar_per_pixel": NBAR, "shape_noise": SIGMA, "seed": SEED,
           "mean_catalogue_size": float(np.mean(sizes)), "expected_catalogue_size": NBAR * npix, "blocks": {}}
    for key, samples in runs.items():
        samples = np.stack(samples)
        mean, sem = samples.mean(axis=0), samples.std(axis=0, ddof=1) / np.sqrt(NREAL)
        want = np.asarray(cls[key])
        with np.errstate(divide="ignore", invalid="ignore"):
            pull = np.where(sem > 0, (mean - want) / sem, 0.0)[..., 2:]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(want != 0, mean / want, np.nan)[..., 2:]
        row = {"mean": mean.tolist(), "sem": sem.tolist(), "input": want.tolist(), "max_abs_pull": float(np.abs(pull).max()),
               "rms_pull": float(np.sqrt(np.mean(pull**2))), "mean_ratio_to_input": float(np.nanmean(ratio)) if np.isfinite(ratio).any() else None}
        out["blocks"]["-".join(str(k) for k in key)] = row
        print(key, {k: v for k, v in row.items() if k not in ("mean", "sem", "input")}, flush=True)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
