"""The two passes of the lognormal mocks that have a size: hx_lognormal_maps at nside 4096 (env NSIDE) and hx_cl_nearest_psd at N = 30
components (env NCOMPS, a list) and lmax 6144 (env LMAX), everything resident in HBM.

Map pass: one map in place and two maps out of place; the whole call by the library's event timer and the kernel alone from its
`lognormal_maps` scope, warmed up, median and min .. max of REPS; bytes read + written over the kernel time against the copy probe of
hx_measure_peaks (which counts read + write bytes too).  Repair: matrices C_l = B B^T / (l + 1)^2 with B square; once as they are
(every matrix is copied through) and once with 10^-2 of the mean diagonal taken off the diagonal of every second l (those are
indefinite and get repaired); the whole call and the `cl_nearest_psd` scope, and the time per repaired matrix.  Results as JSON in OUT
(default profiles/lognormal.json).  DESIGN.md 4.25."""

import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import heracles_amd as hx
from heracles_amd import _lib

NSIDE = int(os.environ.get("NSIDE", "4096"))
LMAX = int(os.environ.get("LMAX", "6144"))
NCOMPS = [int(x) for x in os.environ.get("NCOMPS", "30").split(",")]
REPS = int(os.environ.get("REPS", "7"))
OUT = os.environ.get("OUT", "profiles/lognormal.json")


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def timed(call, scope):
    call()  # warm-up: code objects, scratch
    whole, kernel = [], []
    for _ in range(REPS):
        with _lib.Timer() as t:
            call()
        whole.append(t.ms)
    _lib.profile_enable(True)
    for _ in range(REPS):
        _lib.profile_reset()
        call()
        kernel.append(_lib.profile_get(scope)[1])
    _lib.profile_enable(False)
    return summary(whole), summary(kernel)


def spectra(n, lmax, indefinite):
    rng = np.random.default_rng(n)
    B = rng.standard_normal((lmax + 1, n, n))
    C = np.einsum("lik,ljk->ijl", B, B)
    if indefinite:
        off = 1e-2 * np.einsum("iil->l", C) / n
        off[::2] = 0.0
        C[np.arange(n), np.arange(n)] -= off
    C /= (np.arange(lmax + 1) + 1.0) ** 2
    return np.ascontiguousarray(C[np.triu_indices(n)])


def main():
    hx.init(0)
    L = _lib.load()
    peaks = _lib.measure_peaks()
    print("peaks:", peaks, flush=True)
    rows = []
    npix = 12 * NSIDE * NSIDE
    for nrow, in_place in ((1, True), (2, False)):
        g = torch.randn((nrow, npix), dtype=torch.float64, device="cuda") * 0.3
        out = g if in_place else torch.empty_like(g)
        keep = g.clone() if in_place else None
        s2, lam = np.full(nrow, 0.09), np.full(nrow, 1.0)
        args = (nrow, npix, _lib.ptr(s2), _lib.ptr(lam), _lib.ptr(g), _lib.ptr(out))

        def call():
            if keep is not None:
                g.copy_(keep)  # (in place: start from Gaussian values every time; the copy is outside the kernel scope)
                torch.cuda.synchronize()
            _lib.check(L.hx_lognormal_maps(*args))

        whole, kernel = timed(call, "lognormal_maps")
        nbytes = 16.0 * nrow * npix
        row = {"pass": "lognormal_maps", "nside": NSIDE, "rows": nrow, "in_place": in_place, "call": None if in_place else whole, "kernel": kernel,
               "gb_moved": nbytes / 1e9, "gbs": nbytes / kernel["median_ms"] / 1e6, "of_copy_probe": nbytes / kernel["median_ms"] / 1e6 / peaks["hbm_copy_gbs"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del g, out, keep
        torch.cuda.empty_cache()
    for n in NCOMPS:
        for indefinite in (False, True):
            cl = torch.from_numpy(spectra(n, LMAX, indefinite)).cuda()
            out, change = torch.empty_like(cl), torch.empty(LMAX + 1, dtype=torch.float64, device="cuda")
            args = (n, LMAX, _lib.ptr(cl), -1.0, _lib.ptr(out), _lib.ptr(change))
            whole, kernel = timed(lambda: _lib.check(L.hx_cl_nearest_psd(*args)), "cl_nearest_psd")
            repaired = int((change > 0).sum())
            hx.synalm_components(out, n, seed=1, out=torch.empty((n, (LMAX + 1) * (LMAX + 2) // 2), dtype=torch.complex128, device="cuda"))  # passes the factor
            row = {"pass": "cl_nearest_psd", "ncomp": n, "lmax": LMAX, "repaired": repaired, "largest_change": float(change.max()), "call": whole,
                   "kernel": kernel, "us_per_matrix": kernel["median_ms"] * 1e3 / (LMAX + 1), "input_gb": cl.numel() * 8 / 1e9}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del cl, out, change
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"peaks": peaks, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
