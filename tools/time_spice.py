#!/usr/bin/env python
"""The "Full" jackknife footprint correction over many samples: `correct_footprint_naturalspice` looped over the samples (one
spectrum at a time through hx_cl2corr / hx_corr2cl, numpy in between) against `correct_footprint_naturalspice_batch` (columns of
all samples through hx_cl2corr_cols, hx_xi_ratio, hx_corr2cl_cols).

Shape: BINS tomographic bins x (POS, SHE) with masks VIS / WHT (4 bins: 36 data keys, 36 mask keys), data at --lmax, masks at
--lmax-mask, --samples samples.  Both paths are warmed up once and then timed alternately --reps times (host clock around calls that
end in a device synchronise); medians and the min .. max spread are reported, and the largest difference of the two results.  The two
GEMMs alone: kernel time of the library's own event scopes over the data columns resident in HBM, as FP64 rate and as a share of the
matrix rate `hx_measure_peaks` sustains on this device.

    python tools/time_spice.py [--bins 4] [--lmax 2048] [--lmax-mask 4096] [--samples 32] [--reps 5] [--json F]"""

import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spectra(rng, bins, lmax, lmax_mask, nsamp):
    import heracles_amd as hx

    fields = {"POS": types.SimpleNamespace(mask="VIS", spin=0), "SHE": types.SimpleNamespace(mask="WHT", spin=2)}
    spin = {"POS": 0, "SHE": 2, "VIS": 0, "WHT": 0}

    def keys(f1, f2):
        out = []
        for a, b in ((f1, f1), (f1, f2), (f2, f2)):
            out += [(a, b, i, j) for i in range(1, bins + 1) for j in range(1, bins + 1) if a != b or i <= j]
        return out

    ell, ellm = np.arange(lmax + 1), np.arange(lmax_mask + 1)
    red = 1.0 / (1.0 + ell) ** 2

    def data():
        out = {}
        for k in keys("POS", "SHE"):
            s = (spin[k[0]], spin[k[1]])
            shape = tuple(2 for x in s if x)
            out[k] = hx.Result(rng.standard_normal(shape + (lmax + 1,)) * red, spin=s, axis=-1, ell=ell)
        return out

    # masks: a smooth cap-like spectrum (positive correlation function out to tens of degrees); a jackknife mask is the full one
    # with one region in a hundred removed, up to per-sample noise
    base = np.exp(-ellm * (ellm + 1.0) * (np.radians(8.0) ** 2) / 2) + 1e-4 / (1.0 + ellm) ** 2

    def masks(scale, noise):
        return {k: hx.Result(base * scale * (1.0 + noise * rng.standard_normal(lmax_mask + 1)), spin=(0, 0), axis=-1, ell=ellm)
                for k in keys("VIS", "WHT")}

    mls0 = masks(1.0, 0.0)
    return fields, [data() for _ in range(nsamp)], [masks(0.98, 1e-3) for _ in range(nsamp)], mls0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=4)
    ap.add_argument("--lmax", type=int, default=2048)
    ap.add_argument("--lmax-mask", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch

    import heracles_amd as hx
    from heracles_amd import _lib, transforms as tr, unmixing as um
    from heracles_amd.jackknife import correct_footprint_naturalspice, correct_footprint_naturalspice_batch

    _lib.ensure_init()
    rng = np.random.default_rng(5)
    fields, cls, mljk, mls0 = spectra(rng, a.bins, a.lmax, a.lmax_mask, a.samples)
    ids = list(range(a.samples))

    def loop():
        with np.errstate(all="ignore"):
            return {i: correct_footprint_naturalspice(cls[i], mljk[i], mls0, fields) for i in ids}

    def batch():
        return correct_footprint_naturalspice_batch({i: cls[i] for i in ids}, {i: mljk[i] for i in ids}, mls0, fields)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        _lib.synchronize()
        return time.perf_counter() - t0, out

    _, ref = timed(loop)  # warm-up of both paths (tables of the mask's band limit, code objects)
    _, got = timed(batch)
    worst = 0.0
    for i in ids:
        for k in ref[i]:
            r, g = np.asarray(ref[i][k].array), np.asarray(got[i][k].array)
            worst = max(worst, float(np.nanmax(np.abs(g - r)) / np.nanmax(np.abs(r))))
    t_loop, t_batch = [], []
    for _ in range(a.reps):  # alternated: both see the same neighbours on the host
        t_loop.append(timed(loop)[0])
        t_batch.append(timed(batch)[0])

    # ---- the two GEMMs alone, data columns resident in HBM
    plan = um.spice_plan({k: tuple(r.spin) for k, r in cls[0].items()}, {k: (0, 0) for k in mls0}, fields)
    ncol, nl, n = plan.ncol * a.samples, a.lmax + 1, a.lmax_mask + 1
    fam = np.tile(plan.families, a.samples)
    dev = torch.device("cuda", _lib.device())
    cols = torch.from_numpy(np.concatenate([um._pack_spectra(c, nl) for c in cls])).to(dev)
    xi = torch.empty((ncol, n), dtype=torch.float64, device=dev)
    back = torch.empty((ncol, nl), dtype=torch.float64, device=dev)
    tr.cl2corr_columns(cols, fam, a.lmax_mask, out=xi)
    tr.corr2cl_columns(xi, fam, a.lmax_mask, nl=nl, out=back)
    _lib.profile_enable(True)
    gemm = {}
    for name, call in (("xi_cols_fwd", lambda: tr.cl2corr_columns(cols, fam, a.lmax_mask, out=xi)),
                       ("xi_cols_back", lambda: tr.corr2cl_columns(xi, fam, a.lmax_mask, nl=nl, out=back))):
        ms = []
        for _ in range(a.reps):
            _lib.profile_reset()
            call()
            ms.append(_lib.profile_get(name)[1])
        gemm[name] = ms
    _lib.profile_enable(False)
    peaks = _lib.measure_peaks()
    flop = 2.0 * ncol * nl * n

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    res = {"bins": a.bins, "lmax": a.lmax, "lmax_mask": a.lmax_mask, "samples": a.samples, "reps": a.reps,
           "data_keys": len(cls[0]), "mask_keys": len(mls0), "data_columns_per_sample": plan.ncol, "mask_columns": plan.ncol_mask,
           "loop_seconds": summary(t_loop), "batch_seconds": summary(t_batch),
           "speedup_median": statistics.median(t_loop) / statistics.median(t_batch),
           "max_rel_difference_batch_vs_loop": worst,
           "gemm_columns": ncol, "gemm_flop_each": flop, "fp64_mfma_tflops_sustained": peaks["fp64_mfma_tflops"]}
    for name, ms in gemm.items():
        s = summary(ms)
        res[name + "_ms"] = s
        res[name + "_tflops"] = flop / (s["median"] * 1e-3) / 1e12
        res[name + "_share_of_matrix_rate"] = res[name + "_tflops"] / peaks["fp64_mfma_tflops"]
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    hx.release_caches()


if __name__ == "__main__":
    main()
